// epnn_charges_jvp_xyz_cell: charges and their directional derivative along (vxyz, vstrain, vQ) of a flat coordinate batch
// (kernels and arithmetic: epnn_jvp.hip.h).  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_jvp.hip.h"

// The call shares the pair-list gradient path's state (GradLarge: the weights in plain Keras layout, refreshed when weights_gen
// moves on, and the input / scratch buffers, which keep the size of the largest call of either kind): neither the training state
// nor the forward's plan and pair list are touched.
static int charges_jvp_impl(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                            const EpnnCell *cells, const float *vxyz, const float *vstrain, const float *vQ, float *q_out,
                            float *tq_out) {
    const char *name = "epnn_charges_jvp_xyz_cell";
    GradLarge *gl = grad_large_state(h);
    if (grad_large_weights(h, gl)) return 1;
    const int nx = h->cfg.nx, T = h->cfg.T, A = offsets[B];
    // sweep tasks: 16 resident atoms x one piece of their molecule's partner range (the gradient path's)
    std::vector<int4> tasks;
    int maxp = 1;
    for (int b = 0; b < B; ++b) {
        const int n = offsets[b + 1] - offsets[b], np = gl_pieces(n);
        maxp = std::max(maxp, np);
        for (int a0 = offsets[b]; a0 < offsets[b + 1]; a0 += 16)
            for (int k = 0; k < np; ++k) tasks.push_back(make_int4(a0, b, k, np));
    }
    auto up256 = [](size_t bytes) { return (bytes + 255) & ~size_t(255); };
    // ---- inputs, tangents and the front-end's per-atom counts: one upload
    size_t at = 0;
    auto place = [&](size_t bytes) { const size_t o = at; at += up256(bytes); return o; };
    const size_t o_off = place((size_t)(B + 1) * 4), o_molof = place((size_t)A * 4), o_mflag = place((size_t)B * 4),
                 o_task = place(tasks.size() * sizeof(int4)), o_xyz = place((size_t)A * 12), o_x = place((size_t)A * nx * 4),
                 o_Q = place((size_t)B * 4), o_vQ = place((size_t)B * 4), o_v = place(vxyz ? (size_t)A * 12 : 0),
                 o_E = place(vstrain ? (size_t)B * 36 : 0), o_geo = place(cells ? (size_t)B * sizeof(EpnnCell) : 0), in_bytes = at;
    const size_t o_rowcnt = place((size_t)(A + 1) * 4), o_rowoff = place((size_t)(A + 1) * 4), o_deg = place((size_t)(A + 1) * 4),
                 o_incoff = place((size_t)(A + 1) * 4), o_status = place(16), in_total = at;
    if (gl->pin_in.ensure(in_bytes) || gl->in.ensure(in_total) || gl->pin_out.ensure(64)) return 1;
    char *st = gl->pin_in.as<char>();
    memcpy(st + o_off, offsets, (size_t)(B + 1) * 4);
    int *molof = reinterpret_cast<int *>(st + o_molof), *mflag = reinterpret_cast<int *>(st + o_mflag);
    for (int b = 0; b < B; ++b) {
        mflag[b] = 1;
        for (int a = offsets[b]; a < offsets[b + 1]; ++a) molof[a] = b;
    }
    memcpy(st + o_task, tasks.data(), tasks.size() * sizeof(int4));
    memcpy(st + o_xyz, xyz, (size_t)A * 12);
    memcpy(st + o_x, x, (size_t)A * nx * 4);
    memcpy(st + o_Q, Q, (size_t)B * 4);
    if (vQ) memcpy(st + o_vQ, vQ, (size_t)B * 4);
    else memset(st + o_vQ, 0, (size_t)B * 4);
    if (vxyz) memcpy(st + o_v, vxyz, (size_t)A * 12);
    if (vstrain) memcpy(st + o_E, vstrain, (size_t)B * 36);
    if (cells) memcpy(st + o_geo, cells, (size_t)B * sizeof(EpnnCell));
    char *din = gl->in.as<char>();
    HIPCHK(hipMemcpyAsync(din, st, in_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(din + o_status, 0, 16, h->stream));
    const int *d_moff = reinterpret_cast<const int *>(din + o_off), *d_molof = reinterpret_cast<const int *>(din + o_molof);
    const int4 *d_tasks = reinterpret_cast<const int4 *>(din + o_task);
    const float *d_xyz = reinterpret_cast<const float *>(din + o_xyz), *d_x = reinterpret_cast<const float *>(din + o_x),
                *d_Q = reinterpret_cast<const float *>(din + o_Q), *d_vQ = reinterpret_cast<const float *>(din + o_vQ),
                *d_v = vxyz ? reinterpret_cast<const float *>(din + o_v) : nullptr,
                *d_E = vstrain ? reinterpret_cast<const float *>(din + o_E) : nullptr, *d_geo = reinterpret_cast<const float *>(din + o_geo);
    const EpnnCell *d_cells = reinterpret_cast<const EpnnCell *>(d_geo);
    // ---- pair list: count and prefix sums first, then buffers of exactly that size, then the records and the incidence slots
    FrontArgs F{};
    F.xyz = d_xyz; F.mol_of = d_molof; F.moff = d_moff; F.mflag = reinterpret_cast<const int *>(din + o_mflag);
    F.A = A;
    F.cutoff = (double)h->cfg.cutoff; F.cut2 = cutoff_squared(F.cutoff); F.eta = (double)h->cfg.eta; F.tol = h->cfg.near_tol;
    F.e_dim = h->cfg.e_dim;
    F.mu = h->d_mu.as<double>();
    F.row_cnt = reinterpret_cast<int *>(din + o_rowcnt); F.row_off = reinterpret_cast<int *>(din + o_rowoff);
    F.deg = reinterpret_cast<int *>(din + o_deg); F.inc_off = reinterpret_cast<int *>(din + o_incoff);
    F.status = reinterpret_cast<int *>(din + o_status);
    F.pcap = 0x7fffffff;
    const unsigned rows = (unsigned)((A + 3) / 4), gA = (unsigned)((A + 255) / 256);
    if (cells) hipLaunchKernelGGL(k_front_count_cell, dim3(rows), dim3(256), 0, h->stream, F, d_cells);
    else hipLaunchKernelGGL(k_front_count, dim3(rows), dim3(256), 0, h->stream, F);
    hipLaunchKernelGGL(k_front_scan_both, dim3(1), dim3(1024), 0, h->stream, F);
    HIPCHK(hipGetLastError());
    int *cnt = gl->pin_out.as<int>();
    HIPCHK(hipMemcpyAsync(cnt, F.row_off + A, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cnt + 1, F.inc_off + A, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cnt + 2, F.status, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int np = cnt[0];
    if (cnt[2] != 0) EPNN_FAIL("%s: the pair count overflowed (status %d)", name, cnt[2]);
    if (np < 0 || cnt[1] != 2 * np) EPNN_FAIL("%s: inconsistent pair count (%d pairs, %d incidences)", name, np, cnt[1]);
    const size_t P1 = (size_t)std::max(np, 1), SL = 2 * P1, rowH = (size_t)A * GL_H * 4, rowE = (size_t)A * GL_E * 4;
    at = 0;
    const size_t o_pi = place(P1 * 4), o_pj = place(P1 * 4), o_psym = place(P1 * 4), o_pe = place(P1 * GL_E * 4), o_pwi = place(P1 * 4),
                 o_pwj = place(P1 * 4), o_nbr = place(SL * 4), o_di = place(P1 * 4), o_dj = place(P1 * 4),
                 o_prec = place(2 * (P1 + 256) * sizeof(int4)), o_te = place(P1 * GL_E * 4), o_h = place(2 * rowE), o_th = place(2 * rowE),
                 o_P = place(rowH), o_R = place(rowH), o_Yb = place(rowH), o_Yc = place(rowH), o_tP = place(rowH), o_tR = place(rowH),
                 o_partS = place((size_t)maxp * rowH), o_partT = place((size_t)maxp * rowH), o_slotS = place(SL * GL_H * 4),
                 o_slotT = place(SL * GL_H * 4), o_slotq = place(SL * 4), o_slott = place(SL * 4), o_q = place(2 * (size_t)A * 4),
                 o_tq = place(2 * (size_t)A * 4), o_out = place(((size_t)A * 2 + 1) * 4);
    if (gl->work.ensure(at)) return 1;
    h->stats[0] = np;
    h->stats[1] = 0;
    h->stats[3] = 0;
    h->stats[2] = (int64_t)(at + in_total);                      // device scratch of this call, bytes
    char *dw = gl->work.as<char>();
    auto fp = [&](size_t o) { return reinterpret_cast<float *>(dw + o); };
    auto ip = [&](size_t o) { return reinterpret_cast<int *>(dw + o); };
    F.pcap = (int)P1;
    F.pi = ip(o_pi); F.pj = ip(o_pj); F.psym = ip(o_psym); F.pe = fp(o_pe); F.pwi = fp(o_pwi); F.pwj = fp(o_pwj);
    F.nbr = ip(o_nbr); F.dest_i = ip(o_di); F.dest_j = ip(o_dj); F.prec = reinterpret_cast<int4 *>(dw + o_prec);
    float *out = fp(o_out);                                      // [A] q | [A] tq | bad
    int *bad = reinterpret_cast<int *>(out + 2 * (size_t)A);
    HIPCHK(hipMemsetAsync(bad, 0, 4, h->stream));
    const GlGeom G{d_moff, d_molof, A, N, nx};
    const GlPairs L{F.pi, F.pj, F.dest_i, F.dest_j, F.pe, F.pwi};
    const int *inc = F.inc_off;
    float *te = fp(o_te);
    const unsigned gP = (unsigned)np;
    if (np > 0) {
        if (cells) hipLaunchKernelGGL(k_front_fill_cell, dim3(rows), dim3(256), 0, h->stream, F, d_cells);
        else hipLaunchKernelGGL(k_front_fill, dim3(rows), dim3(256), 0, h->stream, F);
        hipLaunchKernelGGL(k_front_link, dim3((unsigned)std::min<size_t>((P1 + 255) / 256, 1024)), dim3(256), 0, h->stream, F);
        // ---- edge tangents
        const unsigned gp = (unsigned)((np + 255) / 256);
        const double cut = (double)h->cfg.cutoff, eta = (double)h->cfg.eta;
        if (cells) hipLaunchKernelGGL(k_jv_edge<2>, dim3(gp), dim3(256), 0, h->stream, L, np, d_molof, d_xyz, d_geo, d_v, d_E, cut, eta, h->d_mu.as<double>(), te, bad);
        else hipLaunchKernelGGL(k_jv_edge<0>, dim3(gp), dim3(256), 0, h->stream, L, np, d_molof, d_xyz, d_geo, d_v, d_E, cut, eta, h->d_mu.as<double>(), te, bad);
        HIPCHK(hipGetLastError());
    }
    float *hb[2] = {fp(o_h), fp(o_h) + (size_t)A * GL_E}, *thb[2] = {fp(o_th), fp(o_th) + (size_t)A * GL_E};
    float *qb[2] = {fp(o_q), fp(o_q) + A}, *tqb[2] = {fp(o_tq), fp(o_tq) + A};
    float *dP = fp(o_P), *dR = fp(o_R), *Yb = fp(o_Yb), *Yc = fp(o_Yc), *tP = fp(o_tP), *tR = fp(o_tR), *partS = fp(o_partS), *partT = fp(o_partT),
          *slotS = fp(o_slotS), *slotT = fp(o_slotT), *slotq = fp(o_slotq), *slott = fp(o_slott);
    const unsigned nt = (unsigned)tasks.size();
    const dim3 w64(64);
    // the charges before the first EPN step and their tangent: Q / n, vQ / n (every GNN step sees these)
    hipLaunchKernelGGL(k_gl_q0, dim3(gA), dim3(256), 0, h->stream, G, d_Q, qb[0]);
    hipLaunchKernelGGL(k_gl_q0, dim3(gA), dim3(256), 0, h->stream, G, d_vQ, tqb[0]);
    // ---- GNN steps
    for (int t = 0; t < T; ++t) {
        const float *ht = t ? hb[t & 1] : nullptr, *tht = t ? thb[t & 1] : nullptr;
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, gl->msg[t], G, d_x, ht, (const float *)nullptr, d_Q, dP, dR, Yb, Yc);
        hipLaunchKernelGGL(k_jv_proj, dim3(A), w64, 0, h->stream, gl->msg[t], G, tht, (const float *)tqb[0], tP, tR);
        hipLaunchKernelGGL(k_jv_sweep, dim3(nt), w64, 0, h->stream, d_tasks, d_moff, A, gl->msg[t].W2, (const float *)dP, (const float *)tP,
                           (const float *)dR, (const float *)Yb, (const float *)tR, partS, partT, (int)nt);
        if (np > 0)
            hipLaunchKernelGGL(k_jv_gnn_pair, dim3(gP), w64, 0, h->stream, gl->msg[t], L, (const float *)te, (const float *)dP, (const float *)dR,
                               (const float *)tP, (const float *)tR, slotS, slotT);
        hipLaunchKernelGGL(k_jv_gnn_tail, dim3(A), w64, 0, h->stream, gl->msg[t], gl->upd, G, inc, (const float *)partS, (const float *)partT,
                           (const float *)slotS, (const float *)slotT, (const float *)dP, (const float *)tP, ht, tht, hb[(t + 1) & 1],
                           thb[(t + 1) & 1]);
    }
    HIPCHK(hipGetLastError());
    // ---- EPN steps
    const float *feats = hb[T & 1], *tfeats = thb[T & 1];
    for (int t = 0; t < T; ++t) {
        const float *qt = qb[t & 1], *tqt = tqb[t & 1];
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, gl->pas[t], G, d_x, feats, qt, d_Q, dP, dR, (float *)nullptr, (float *)nullptr);
        hipLaunchKernelGGL(k_jv_proj, dim3(A), w64, 0, h->stream, gl->pas[t], G, tfeats, tqt, tP, tR);
        if (np > 0)
            hipLaunchKernelGGL(k_jv_epn_pair, dim3(gP), w64, 0, h->stream, gl->pas[t], L, (const float *)te, (const float *)dP, (const float *)dR,
                               (const float *)tP, (const float *)tR, slotq, slott);
        hipLaunchKernelGGL(k_gl_epn_atom, dim3(gA), dim3(256), 0, h->stream, A, inc, (const float *)slotq, qt, qb[(t + 1) & 1]);
        hipLaunchKernelGGL(k_gl_epn_atom, dim3(gA), dim3(256), 0, h->stream, A, inc, (const float *)slott, tqt, tqb[(t + 1) & 1]);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, qb[T & 1], (size_t)A * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(out + A, tqb[T & 1], (size_t)A * 4, hipMemcpyDeviceToDevice, h->stream));
    const size_t nback = (size_t)A * 2 + 1;
    if (gl->pin_out.ensure(nback * 4)) return 1;
    float *back = gl->pin_out.as<float>();
    HIPCHK(hipMemcpyAsync(back, out, nback * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int flag = reinterpret_cast<const int *>(back)[2 * (size_t)A];
    if (flag & 2) EPNN_FAIL("%s: the pair list is not symmetric", name);
    if (flag != 0)
        EPNN_FAIL("%s: two atoms of a molecule%s coincide (distance 0: the edge features have no derivative there)", name,
                  cells ? " or their periodic images" : "");
    memcpy(q_out, back, (size_t)A * 4);
    memcpy(tq_out, back + A, (size_t)A * 4);
    return 0;
}

extern "C" int epnn_charges_jvp_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                         const float *Q, const float *cell, const float *vxyz, const float *vstrain, const float *vQ,
                                         float *q_out, float *tq_out) {
    const char *name = "epnn_charges_jvp_xyz_cell";
    if (!h || !offsets || !xyz || !x || !Q || !q_out || !tq_out) EPNN_FAIL("%s: null argument", name);
    if (B < 1 || N < 1 || offsets[0] != 0) EPNN_FAIL("%s: B and N must be positive and offsets[0] must be 0", name);
    for (int b = 0; b < B; ++b)
        if (offsets[b + 1] - offsets[b] > N || offsets[b + 1] - offsets[b] < 1) EPNN_FAIL("%s: molecule %d does not fit N=%d", name, b, N);
    EPNN_NOT_FUSED_ONLY(h, name);
    std::vector<EpnnCell> cells;
    if (cell && check_cell(B, cell, (double)h->cfg.cutoff, name, cells)) return 1;
    if (h->upd_generic) EPNN_FAIL("%s is built for update layers [32, 32] only (epnn_set_update_layers changed them)", name);
    if (h->part_world != 1) EPNN_FAIL("%s does not run on a partitioned handle (epnn_set_partition)", name);
    HIPCHK(hipSetDevice(h->device));
    if (h->pending.active && finish_forward(h)) return 1;
    // the weights epnn_forward_xyz would use: a training step still in flight is waited for, device masters it has updated are
    // pulled into the host copies (what any inference call does first)
    if (train_quiesce(h) || pack_weights(h)) return 1;
    return charges_jvp_impl(h, B, N, offsets, xyz, x, Q, cell ? cells.data() : nullptr, vxyz, vstrain, vQ, q_out, tq_out);
}
