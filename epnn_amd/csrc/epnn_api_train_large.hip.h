// epnn_train_step_xyz_cell: a training step on open molecules or periodic cells, on the dense path (train_step_xyz_impl) or from
// the pair list (option "train_path"; kernels: epnn_train_large.hip.h).  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_train_large.hip.h"

// The pair-list step: the checkpointed forward and the activation backward of charges_vjp_large_impl with the seed gq = 2 (q - y),
// without its coordinate tail, with step 0 run in full (a_i of step 0 does not depend on the coordinates, but on the weights it does)
// and every kernel keeping the rows of its weight gradients (the TAPE instances of the one backward, epnn_vjp_multi.hip.h, at K = 1).  It reads the training state's device masters where they are
// (the flat vector has the layout GlPair / GlUpd point into), adds into the state's gradient vector, and returns when all of it is
// done.  Inputs, pair list and scratch are those of the gradient path (GradLarge).
static int train_step_large_impl(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                 const HostGeo &geo, const float *y, float *q_out, float *loss_out, int apply) {
    const char *name = "epnn_train_step_xyz_cell";
    TrainState *ts = train_state(h);
    GradLarge *gl = grad_large_state(h);
    const int T = h->cfg.T, A = offsets[B], F = h->cfg.nx + GL_E + 1;
    if (gl_check_shapes(name, T, F, ts->msg, ts->pas, ts->upd)) return 1;
    const float *theta = ts->theta.as<float>();
    GlPair msg[EPNN_MAXT], pas[EPNN_MAXT];
    for (int t = 0; t < T; ++t) {
        const TDense *M = ts->msg[t], *P = ts->pas[t];
        gl_point_pair(msg[t], theta, M[0].offW, M[0].offB, M[1].offW, M[1].offB, M[2].offW, M[2].offB, F);
        gl_point_pair(pas[t], theta, P[0].offW, P[0].offB, P[1].offW, P[1].offB, P[2].offW, P[2].offB, F);
    }
    const GlUpd upd{theta + ts->upd[0].offW, theta + ts->upd[0].offB, theta + ts->upd[1].offW, theta + ts->upd[1].offB,
                    theta + ts->upd[2].offW, theta + ts->upd[2].offB};
    const GlSpan span_y{y, (size_t)A * 4, false};
    GlCall c;
    if (gl_call_count(h, gl, "epnn_train_step_xyz_cell (pair-list path)", B, N, offsets, xyz, x, Q, geo, &span_y, 1, c)) return 1;
    const int np = c.np;
    const size_t P1 = c.P1, SL = 2 * P1, rowH = (size_t)A * GL_H * 4, rowE = (size_t)A * GL_E * 4, maxp = (size_t)c.maxp;
    const unsigned nt = c.nt;
    const int run = (int)((nt + TL_NW - 1) / TL_NW);
    const unsigned nw = (nt + run - 1) / run;                       // wavefronts of the weight-gradient sweep
    const size_t tape_rows = 4 * P1 + (size_t)A;                    // pair rows (r3 lives in the second half of z1's during the EPN stack), then atom rows
    const size_t o_h = c.place((size_t)(T + 1) * rowE), o_S = c.place((size_t)T * rowH),
                 o_q = c.place((size_t)(T + 1) * A * 4), o_P = c.place(rowH), o_R = c.place(rowH), o_Yb = c.place(rowH), o_Yc = c.place(rowH),
                 o_dS = c.place(rowH), o_partP = c.place(maxp * rowH), o_partR = c.place(maxp * rowH),
                 o_slotP = c.place(SL * GL_H * 4), o_slotR = c.place(SL * GL_H * 4), o_slotq = c.place(SL * 4), o_gh = c.place(rowE),
                 o_ghp = c.place(rowE), o_out = c.place(((size_t)A * 3 + 1) * 4),
                 o_tz = c.place(tape_rows * GL_H * 4), o_td = c.place(tape_rows * GL_H * 4), o_tdz = c.place(P1 * GL_H * 4),
                 o_u0 = c.place((size_t)A * (GL_E + GL_H) * 4), o_u1 = c.place(rowH), o_u2 = c.place(rowH), o_ud2 = c.place(rowH),
                 o_ud1 = c.place(rowH), o_gm = c.place(rowH), o_dv = c.place(2 * rowH), o_arow = c.place(2 * rowH),
                 o_part = c.place((size_t)TL_MAXJOBS * TL_G * TL_PS * 4), o_wpart = c.place((size_t)nw * (GL_H * GL_H + GL_H) * 4);
    if (gl_call_fill(h, gl, c, gl->in.cap)) return 1;
    const unsigned gP = (unsigned)np, gA = c.gA;
    const GlGeom &G = c.G;
    const GlPairs &L = c.L;
    const int *inc = c.inc;
    const float *d_x = c.d_x, *d_Q = c.d_Q, *d_y = c.d_extra[0];
    float *hck = c.fp(o_h), *Sck = c.fp(o_S), *qck = c.fp(o_q), *dP = c.fp(o_P), *dR = c.fp(o_R), *Yb = c.fp(o_Yb), *Yc = c.fp(o_Yc), *dS = c.fp(o_dS),
          *partP = c.fp(o_partP), *partR = c.fp(o_partR), *slotP = c.fp(o_slotP), *slotR = c.fp(o_slotR), *slotq = c.fp(o_slotq), *gh = c.fp(o_gh),
          *ghp = c.fp(o_ghp), *out = c.fp(o_out), *arow = c.fp(o_arow), *part = c.fp(o_part), *wpart = c.fp(o_wpart);
    GlTape K{};
    K.z1 = c.fp(o_tz); K.d2 = c.fp(o_td); K.dz = c.fp(o_tdz); K.r3 = K.z1 + 2 * P1 * GL_H;
    K.u0 = c.fp(o_u0); K.u1 = c.fp(o_u1); K.u2 = c.fp(o_u2); K.ud2 = c.fp(o_ud2); K.ud1 = c.fp(o_ud1); K.gm = c.fp(o_gm); K.dv = c.fp(o_dv);
    K.pad0 = 4 * (size_t)np;
    const size_t nH = (size_t)A * GL_H, nE = (size_t)A * GL_E;
    const dim3 w64(64);
    if (gl_forward_ckpt(h, c, msg, pas, upd, hck, Sck, qck, dP, dR, Yb, Yc, partP, slotP, slotq)) return 1;
    const float *feats = hck + T * nE;
    // ---- loss and seed
    float *gq = out, *q_fin = out + A, *term = out + 2 * (size_t)A;       // [A] gq | [A] q | [A] loss terms | bad
    int *bad = reinterpret_cast<int *>(out + 3 * (size_t)A);
    float *grad = ts->grad.as<float>();
    HIPCHK(hipMemsetAsync(grad, 0, (size_t)ts->P * 4, h->stream));
    HIPCHK(hipMemsetAsync(gh, 0, nE * 4, h->stream));
    HIPCHK(hipMemsetAsync(bad, 0, 4, h->stream));
    HIPCHK(hipMemcpyAsync(q_fin, qck + (size_t)T * A, (size_t)A * 4, hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(k_tl_seed, dim3(gA), dim3(256), 0, h->stream, A, (const float *)q_fin, d_y, gq, term);
    if (np > 0) hipLaunchKernelGGL(k_tl_check_pairs, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream, L, np, bad);
    // the weight gradients of one phase: its jobs in one launch, their partials added into the gradient vector in another
    TlJobs J{};
    TlRed Rd{};
    int nj = 0, nr = 0;
    auto job = [&](const float *X, int xs, int Kd, const float *Y, int ys, int O, size_t nrows, int offW, int offB, float bscale = 1.f) {
        J.j[nj] = TlJob{X, Y, Kd, O, xs, ys, (long long)nrows};
        const long long src = (long long)nj * TL_G * TL_PS;
        if (offW >= 0 && Kd > 0) {
            Rd.dst[nr] = offW; Rd.len[nr] = Kd * O; Rd.nblk[nr] = TL_G; Rd.stride[nr] = TL_PS; Rd.src[nr] = src; Rd.scale[nr] = 1.f;
            nr += 1;
        }
        if (offB >= 0) {
            Rd.dst[nr] = offB; Rd.len[nr] = O; Rd.nblk[nr] = TL_G; Rd.stride[nr] = TL_PS; Rd.src[nr] = src + Kd * O; Rd.scale[nr] = bscale;
            nr += 1;
        }
        nj += 1;
    };
    auto flush = [&]() {
        int maxlen = 0;
        for (int k = 0; k < nr; ++k) maxlen = std::max(maxlen, Rd.len[k]);
        hipLaunchKernelGGL(k_tl_outer, dim3(TL_G, (unsigned)nj), dim3(256), 0, h->stream, J, part);
        hipLaunchKernelGGL(k_tl_reduce, dim3((unsigned)((maxlen + 63) / 64), (unsigned)nr), dim3(1024), 0, h->stream, Rd, (const float *)part, grad);
        nj = 0;
        nr = 0;
    };
    const unsigned gA64 = (unsigned)(((size_t)A * 64 + 255) / 256);
    // ---- backward: EPN stack
    for (int t = T - 1; t >= 0; --t) {
        const float *qt = qck + (size_t)t * A;
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, pas[t], G, d_x, feats, qt, d_Q, dP, dR, (float *)nullptr, (float *)nullptr);
        hipLaunchKernelGGL(k_tl_arow, dim3(gA64), dim3(256), 0, h->stream, G, d_x, feats, qt, d_Q, arow);
        if (np > 0)
            hipLaunchKernelGGL((k_gvm_epn_pair<1, true>), dim3(gP), w64, 0, h->stream, pas[t], L, 1, A, P1, SL, (const float *)dP, (const float *)dR,
                               (const float *)gq, slotP, slotR, (float *)nullptr, K);
        hipLaunchKernelGGL((k_gvm_epn_atom_bwd<1, true>), dim3(A), w64, 0, h->stream, pas[t], G, 1, SL, inc, (const float *)slotP,
                           (const float *)slotR, gh, gq, K);
        const TDense *D = ts->pas[t];
        job(arow, 64, F, K.dv, 64, GL_H, A, D[0].offW, D[0].offB);                                   // Wi, b1
        job(arow, 64, F, K.dv + GL_H, 64, GL_H, A, D[0].offW + F * GL_H, -1);                        // Wj
        job(L.pe, GL_E, GL_E, K.dz, GL_H, GL_H, np, D[0].offW + 2 * F * GL_H, -1);                   // We
        job(K.z1, GL_H, GL_H, K.d2, GL_H, GL_H, 2 * (size_t)np, D[1].offW, D[1].offB);               // W2, b2
        job(nullptr, 0, 0, K.r3, GL_H, GL_H, 2 * (size_t)np, -1, D[2].offW);                         // W3 [32][1]
        flush();
    }
    HIPCHK(hipGetLastError());
    // ---- backward: GNN steps
    for (int t = T - 1; t >= 0; --t) {
        const float *ht = t ? hck + t * nE : nullptr;
        hipLaunchKernelGGL((k_gvm_upd_bwd<1, true>), dim3(A), w64, 0, h->stream, msg[t], upd, G, 1, ht, (const float *)(Sck + t * nH),
                           (const float *)gh, ghp, dS, K);
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, msg[t], G, d_x, ht, (const float *)nullptr, d_Q, dP, dR, Yb, Yc);
        hipLaunchKernelGGL(k_tl_arow, dim3(gA64), dim3(256), 0, h->stream, G, d_x, ht, (const float *)nullptr, d_Q, arow);
        hipLaunchKernelGGL((k_gl_sweep<1, 1, 1>), dim3(nw), w64, 0, h->stream, c.d_tasks, c.d_moff, A, msg[t].W2, (const float *)dP, (const float *)dR,
                           (const float *)Yb, (const float *)dS, (size_t)0, partP, (size_t)0, (int)nt, run, wpart);
        hipLaunchKernelGGL(k_gl_sweep<2>, dim3(nt), w64, 0, h->stream, c.d_tasks, c.d_moff, A, msg[t].W2, (const float *)dR, (const float *)dP,
                           (const float *)Yc, (const float *)dS, (size_t)0, partR, (size_t)0, (int)nt, 1, (float *)nullptr);
        const TDense *D = ts->msg[t];
        {                                                          // W2, b2 of all pairs: the sweep's partials
            TlRed Rs{};
            Rs.dst[0] = D[1].offW; Rs.len[0] = GL_H * GL_H; Rs.src[0] = 0;
            Rs.dst[1] = D[1].offB; Rs.len[1] = GL_H; Rs.src[1] = GL_H * GL_H;
            for (int k = 0; k < 2; ++k) { Rs.nblk[k] = (int)nw; Rs.stride[k] = GL_H * GL_H + GL_H; Rs.scale[k] = 1.f; }
            hipLaunchKernelGGL(k_tl_reduce, dim3(GL_H * GL_H / 64, 2), dim3(1024), 0, h->stream, Rs, (const float *)wpart, grad);
        }
        if (np > 0)
            hipLaunchKernelGGL((k_gvm_gnn_pair<1, true>), dim3(gP), w64, 0, h->stream, msg[t], L, 1, A, P1, SL, (const float *)dP, (const float *)dR,
                               (const float *)dS, slotP, slotR, (float *)nullptr, K);
        hipLaunchKernelGGL((k_gvm_gnn_atom_bwd<1, true>), dim3(A), w64, 0, h->stream, msg[t], G, 1, (size_t)0, SL, inc, (const float *)partP,
                           (const float *)partR, (const float *)slotP, (const float *)slotR, (const float *)dP, (const float *)dS, ghp, K);
        job(K.u0, GL_E + GL_H, GL_E + GL_H, K.ud1, GL_H, GL_H, A, ts->upd[0].offW, ts->upd[0].offB);  // update MLP
        job(K.u1, GL_H, GL_H, K.ud2, GL_H, GL_H, A, ts->upd[1].offW, ts->upd[1].offB);
        job(K.u2, GL_H, GL_H, gh, GL_E, GL_E, A, ts->upd[2].offW, ts->upd[2].offB);
        job(Sck + t * nH, GL_H, GL_H, K.gm, GL_H, GL_H, A, D[2].offW, D[2].offB, (float)N);          // W3, N b3
        job(arow, 64, F, K.dv, 64, GL_H, A, D[0].offW, D[0].offB);                                    // Wi, b1
        job(arow, 64, F, K.dv + GL_H, 64, GL_H, A, D[0].offW + F * GL_H, -1);                         // Wj
        job(L.pe, GL_E, GL_E, K.dz, GL_H, GL_H, np, D[0].offW + 2 * F * GL_H, -1);                    // We
        job(K.z1, GL_H, GL_H, K.d2, GL_H, GL_H, 4 * (size_t)np + A, D[1].offW, D[1].offB);            // W2, b2: corrections and padded partners
        flush();
        std::swap(gh, ghp);
    }
    HIPCHK(hipGetLastError());
    // q | loss terms | flag: one download, looked at before the optimizer may touch the weights
    const size_t nback = 2 * (size_t)A + 1;
    if (gl->pin_out.ensure(nback * 4)) return 1;
    float *back = gl->pin_out.as<float>();
    HIPCHK(hipMemcpyAsync(back, q_fin, nback * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (reinterpret_cast<const int *>(back)[2 * (size_t)A] != 0) EPNN_FAIL("%s (pair-list path): the pair list is not symmetric", name);
    if (apply) {
        if (train_apply(h)) return 1;
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (q_out) memcpy(q_out, back, (size_t)A * 4);
    if (loss_out) {
        double s = 0;
        for (int a = 0; a < A; ++a) s += back[(size_t)A + a];
        *loss_out = (float)s;
    }
    return 0;
}

static int train_step_xyz_cell_impl(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                    const float *cell, const float *y_flat, float *q_out_flat, float *loss_out, int apply) {
    const char *name = "epnn_train_step_xyz_cell";
    if (!h || !offsets || !xyz || !x || !Q || !y_flat) EPNN_FAIL("%s: null argument", name);
    EPNN_NOT_FUSED_ONLY(h, name);
    HIPCHK(hipSetDevice(h->device));
    if (h->pending.active && finish_forward(h)) return 1;
    if (check_flat_batch(name, B, N, offsets)) return 1;
    GeoArg arg;                                                  // (a null cell: open molecules)
    if (cell && arg.cell(B, cell, (double)h->cfg.cutoff, name)) return 1;
    if (!train_state(h)->ready) EPNN_FAIL("train step: call epnn_train_init first");
    // "train_path": 0 = by size, 1 = the dense path, 2 = the pair-list path (refused where it is not built)
    if (h->opt_train_path == 2 && h->upd_generic)
        EPNN_FAIL("%s: train_path = 2 (pair-list path) is built for update layers [32, 32] only (epnn_set_update_layers changed them)", name);
    if (h->opt_train_path == 2 && h->part_world != 1)
        EPNN_FAIL("%s: train_path = 2 (pair-list path) does not run on a partitioned handle (epnn_set_partition)", name);
    if (h->opt_train_path == 2 || (h->opt_train_path == 0 && grad_large_possible(h) && grad_large_auto(B, N))) {
        if (train_quiesce(h)) return 1;                          // a dense "train_async" step may still be reading the masters' gradients
        return train_step_large_impl(h, B, N, offsets, xyz, x, Q, arg.geo, y_flat, q_out_flat, loss_out, apply);
    }
    return train_step_xyz_impl(h, B, N, offsets, xyz, x, Q, y_flat, q_out_flat, loss_out, apply, arg.geo);
}
extern "C" int epnn_train_step_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                        const float *Q, const float *cell, const float *y_flat, float *q_out_flat, float *loss_out,
                                        int apply) {
    if (!train_step_guarded(h, apply)) return train_step_xyz_cell_impl(h, B, N, offsets, xyz, x, Q, cell, y_flat, q_out_flat, loss_out, apply);
    h->guard_pending = true;
    return comm_guard_exit(h, train_step_xyz_cell_impl(h, B, N, offsets, xyz, x, Q, cell, y_flat, q_out_flat, loss_out, apply),
                           "train step (gradient all-reduce)");
}
