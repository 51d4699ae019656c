// epnn_train_step_xyz_cell: a training step on open molecules or periodic cells, on the dense path (train_step_xyz_impl) or from
// the pair list (option "train_path"; kernels: epnn_train_large.hip.h).  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_train_large.hip.h"

// The pair-list step: the checkpointed forward and the activation backward of charges_vjp_large_impl with the seed gq = 2 (q - y),
// without its coordinate tail, with step 0 run in full (a_i of step 0 does not depend on the coordinates, but on the weights it does)
// and every kernel keeping the rows of its weight gradients (GlTape).  It reads the training state's device masters where they are
// (the flat vector has the layout GlPair / GlUpd point into), adds into the state's gradient vector, and returns when all of it is
// done.  Inputs, pair list and scratch are those of the gradient path (GradLarge).
static int train_step_large_impl(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                 const EpnnCell *cells, const float *y, float *q_out, float *loss_out, int apply) {
    const char *name = "epnn_train_step_xyz_cell";
    TrainState *ts = train_state(h);
    GradLarge *gl = grad_large_state(h);
    const int nx = h->cfg.nx, T = h->cfg.T, A = offsets[B], F = nx + GL_E + 1;
    for (int t = 0; t < T; ++t)
        for (int pass = 0; pass < 2; ++pass) {
            const TDense *L = pass ? ts->pas[t] : ts->msg[t];
            if (L[0].n_in != 2 * F + GL_E || L[0].n_out != GL_H || L[1].n_in != GL_H || L[1].n_out != GL_H || L[2].n_in != GL_H ||
                L[2].n_out != (pass ? 1 : GL_H))
                EPNN_FAIL("%s (pair-list path): unexpected shape of a %s MLP", name, pass ? "pass" : "message");
        }
    if (ts->upd[0].n_in != GL_E + GL_H || ts->upd[0].n_out != GL_H || ts->upd[1].n_out != GL_H || ts->upd[2].n_out != GL_E)
        EPNN_FAIL("%s (pair-list path): unexpected shape of the update MLP", name);
    const float *theta = ts->theta.as<float>();
    GlPair msg[EPNN_MAXT], pas[EPNN_MAXT];
    for (int t = 0; t < T; ++t)
        for (int pass = 0; pass < 2; ++pass) {
            const TDense *L = pass ? ts->pas[t] : ts->msg[t];
            GlPair &M = pass ? pas[t] : msg[t];
            M.Wi = theta + L[0].offW; M.Wj = M.Wi + (size_t)F * GL_H; M.We = M.Wj + (size_t)F * GL_H;
            M.b1 = theta + L[0].offB; M.W2 = theta + L[1].offW; M.b2 = theta + L[1].offB; M.W3 = theta + L[2].offW; M.b3 = theta + L[2].offB;
        }
    const GlUpd upd{theta + ts->upd[0].offW, theta + ts->upd[0].offB, theta + ts->upd[1].offW, theta + ts->upd[1].offB,
                    theta + ts->upd[2].offW, theta + ts->upd[2].offB};
    // sweep tasks: 16 resident atoms x one piece of their molecule's partner range
    std::vector<int4> tasks;
    int maxp = 1;
    for (int b = 0; b < B; ++b) {
        const int n = offsets[b + 1] - offsets[b], np = gl_pieces(n);
        maxp = std::max(maxp, np);
        for (int a0 = offsets[b]; a0 < offsets[b + 1]; a0 += 16)
            for (int k = 0; k < np; ++k) tasks.push_back(make_int4(a0, b, k, np));
    }
    auto up256 = [](size_t bytes) { return (bytes + 255) & ~size_t(255); };
    // ---- inputs and the front-end's per-atom counts: one upload
    size_t at = 0;
    auto place = [&](size_t bytes) { const size_t o = at; at += up256(bytes); return o; };
    const size_t o_off = place((size_t)(B + 1) * 4), o_molof = place((size_t)A * 4), o_mflag = place((size_t)B * 4),
                 o_task = place(tasks.size() * sizeof(int4)), o_xyz = place((size_t)A * 12), o_x = place((size_t)A * nx * 4),
                 o_Q = place((size_t)B * 4), o_y = place((size_t)A * 4), o_geo = place(cells ? (size_t)B * sizeof(EpnnCell) : 0),
                 in_bytes = at;
    const size_t o_rowcnt = place((size_t)(A + 1) * 4), o_rowoff = place((size_t)(A + 1) * 4), o_deg = place((size_t)(A + 1) * 4),
                 o_incoff = place((size_t)(A + 1) * 4), o_status = place(16);
    if (gl->pin_in.ensure(in_bytes) || gl->in.ensure(at) || gl->pin_out.ensure(64)) return 1;
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
    memcpy(st + o_y, y, (size_t)A * 4);
    if (cells) memcpy(st + o_geo, cells, (size_t)B * sizeof(EpnnCell));
    char *din = gl->in.as<char>();
    HIPCHK(hipMemcpyAsync(din, st, in_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(din + o_status, 0, 16, h->stream));
    const int *d_moff = reinterpret_cast<const int *>(din + o_off), *d_molof = reinterpret_cast<const int *>(din + o_molof);
    const int4 *d_tasks = reinterpret_cast<const int4 *>(din + o_task);
    const float *d_xyz = reinterpret_cast<const float *>(din + o_xyz), *d_x = reinterpret_cast<const float *>(din + o_x),
                *d_Q = reinterpret_cast<const float *>(din + o_Q), *d_y = reinterpret_cast<const float *>(din + o_y);
    const EpnnCell *d_cells = reinterpret_cast<const EpnnCell *>(din + o_geo);
    // ---- pair list: count and prefix sums first, then buffers of exactly that size, then the records and the incidence slots
    FrontArgs FA{};
    FA.xyz = d_xyz; FA.mol_of = d_molof; FA.moff = d_moff; FA.mflag = reinterpret_cast<const int *>(din + o_mflag);
    FA.A = A;
    FA.cutoff = (double)h->cfg.cutoff; FA.cut2 = cutoff_squared(FA.cutoff); FA.eta = (double)h->cfg.eta; FA.tol = h->cfg.near_tol;
    FA.e_dim = h->cfg.e_dim;
    FA.mu = h->d_mu.as<double>();
    FA.row_cnt = reinterpret_cast<int *>(din + o_rowcnt); FA.row_off = reinterpret_cast<int *>(din + o_rowoff);
    FA.deg = reinterpret_cast<int *>(din + o_deg); FA.inc_off = reinterpret_cast<int *>(din + o_incoff);
    FA.status = reinterpret_cast<int *>(din + o_status);
    FA.pcap = 0x7fffffff;
    const unsigned rows = (unsigned)((A + 3) / 4), gA = (unsigned)((A + 255) / 256);
    if (cells) hipLaunchKernelGGL(k_front_count_cell, dim3(rows), dim3(256), 0, h->stream, FA, d_cells);
    else hipLaunchKernelGGL(k_front_count, dim3(rows), dim3(256), 0, h->stream, FA);
    hipLaunchKernelGGL(k_front_scan_both, dim3(1), dim3(1024), 0, h->stream, FA);
    HIPCHK(hipGetLastError());
    int *cnt = gl->pin_out.as<int>();
    HIPCHK(hipMemcpyAsync(cnt, FA.row_off + A, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cnt + 1, FA.inc_off + A, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cnt + 2, FA.status, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int np = cnt[0];
    if (cnt[2] != 0) EPNN_FAIL("%s (pair-list path): the pair count overflowed (status %d)", name, cnt[2]);
    if (np < 0 || cnt[1] != 2 * np) EPNN_FAIL("%s (pair-list path): inconsistent pair count (%d pairs, %d incidences)", name, np, cnt[1]);
    const size_t P1 = (size_t)std::max(np, 1), SL = 2 * P1, rowH = (size_t)A * GL_H * 4, rowE = (size_t)A * GL_E * 4;
    const unsigned nt = (unsigned)tasks.size();
    const int run = (int)((nt + TL_NW - 1) / TL_NW);
    const unsigned nw = (nt + run - 1) / run;                       // wavefronts of the weight-gradient sweep
    const size_t tape_rows = 4 * P1 + (size_t)A;                    // pair rows (r3 lives in the second half of z1's during the EPN stack), then atom rows
    at = 0;
    const size_t o_pi = place(P1 * 4), o_pj = place(P1 * 4), o_psym = place(P1 * 4), o_pe = place(P1 * GL_E * 4), o_pwi = place(P1 * 4),
                 o_pwj = place(P1 * 4), o_nbr = place(SL * 4), o_di = place(P1 * 4), o_dj = place(P1 * 4),
                 o_prec = place(2 * (P1 + 256) * sizeof(int4)), o_h = place((size_t)(T + 1) * rowE), o_S = place((size_t)T * rowH),
                 o_q = place((size_t)(T + 1) * A * 4), o_P = place(rowH), o_R = place(rowH), o_Yb = place(rowH), o_Yc = place(rowH),
                 o_dS = place(rowH), o_partP = place((size_t)maxp * rowH), o_partR = place((size_t)maxp * rowH),
                 o_slotP = place(SL * GL_H * 4), o_slotR = place(SL * GL_H * 4), o_slotq = place(SL * 4), o_gh = place(rowE),
                 o_ghp = place(rowE), o_out = place(((size_t)A * 3 + 1) * 4),
                 o_tz = place(tape_rows * GL_H * 4), o_td = place(tape_rows * GL_H * 4), o_tdz = place(P1 * GL_H * 4),
                 o_u0 = place((size_t)A * (GL_E + GL_H) * 4), o_u1 = place(rowH), o_u2 = place(rowH), o_ud2 = place(rowH),
                 o_ud1 = place(rowH), o_gm = place(rowH), o_dv = place(2 * rowH), o_arow = place(2 * rowH),
                 o_part = place((size_t)TL_MAXJOBS * TL_G * TL_PS * 4), o_wpart = place((size_t)nw * (GL_H * GL_H + GL_H) * 4);
    if (gl->work.ensure(at)) return 1;
    h->stats[0] = np;
    h->stats[1] = 0;
    h->stats[3] = 0;
    h->stats[2] = (int64_t)(at + gl->in.cap);                    // device scratch of this call, bytes
    char *dw = gl->work.as<char>();
    auto fp = [&](size_t o) { return reinterpret_cast<float *>(dw + o); };
    auto ip = [&](size_t o) { return reinterpret_cast<int *>(dw + o); };
    FA.pcap = (int)P1;
    FA.pi = ip(o_pi); FA.pj = ip(o_pj); FA.psym = ip(o_psym); FA.pe = fp(o_pe); FA.pwi = fp(o_pwi); FA.pwj = fp(o_pwj);
    FA.nbr = ip(o_nbr); FA.dest_i = ip(o_di); FA.dest_j = ip(o_dj); FA.prec = reinterpret_cast<int4 *>(dw + o_prec);
    if (np > 0) {
        if (cells) hipLaunchKernelGGL(k_front_fill_cell, dim3(rows), dim3(256), 0, h->stream, FA, d_cells);
        else hipLaunchKernelGGL(k_front_fill, dim3(rows), dim3(256), 0, h->stream, FA);
        hipLaunchKernelGGL(k_front_link, dim3((unsigned)std::min<size_t>((P1 + 255) / 256, 1024)), dim3(256), 0, h->stream, FA);
        HIPCHK(hipGetLastError());
    }
    const GlGeom G{d_moff, d_molof, A, N, nx};
    const GlPairs L{FA.pi, FA.pj, FA.dest_i, FA.dest_j, FA.pe, FA.pwi};
    const int *inc = FA.inc_off;
    float *hck = fp(o_h), *Sck = fp(o_S), *qck = fp(o_q), *dP = fp(o_P), *dR = fp(o_R), *Yb = fp(o_Yb), *Yc = fp(o_Yc), *dS = fp(o_dS),
          *partP = fp(o_partP), *partR = fp(o_partR), *slotP = fp(o_slotP), *slotR = fp(o_slotR), *slotq = fp(o_slotq), *gh = fp(o_gh),
          *ghp = fp(o_ghp), *out = fp(o_out), *arow = fp(o_arow), *part = fp(o_part), *wpart = fp(o_wpart);
    GlTape K{};
    K.z1 = fp(o_tz); K.d2 = fp(o_td); K.dz = fp(o_tdz); K.r3 = K.z1 + 2 * P1 * GL_H;
    K.u0 = fp(o_u0); K.u1 = fp(o_u1); K.u2 = fp(o_u2); K.ud2 = fp(o_ud2); K.ud1 = fp(o_ud1); K.gm = fp(o_gm); K.dv = fp(o_dv);
    K.pad0 = 4 * (size_t)np;
    const size_t nH = (size_t)A * GL_H, nE = (size_t)A * GL_E;
    const unsigned gP = (unsigned)np;
    const dim3 w64(64);
    // ---- forward with checkpoints
    for (int t = 0; t < T; ++t) {
        const float *ht = t ? hck + t * nE : nullptr;
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, msg[t], G, d_x, ht, (const float *)nullptr, d_Q, dP, dR, Yb, Yc);
        hipLaunchKernelGGL(k_gl_sweep<0>, dim3(nt), w64, 0, h->stream, d_tasks, d_moff, A, msg[t].W2, (const float *)dP, (const float *)dR,
                           (const float *)Yb, (const float *)nullptr, partP, (int)nt, 1, (float *)nullptr);
        if (np > 0)
            hipLaunchKernelGGL(k_gl_gnn_pair<0>, dim3(gP), w64, 0, h->stream, msg[t], L, (const float *)dP, (const float *)dR,
                               (const float *)nullptr, slotP, (float *)nullptr, (float *)nullptr, GlTape{});
        hipLaunchKernelGGL(k_gl_gnn_tail, dim3(A), w64, 0, h->stream, msg[t], upd, G, inc, (const float *)partP, (const float *)slotP,
                           (const float *)dP, ht, Sck + t * nH, hck + (t + 1) * nE);
    }
    HIPCHK(hipGetLastError());
    const float *feats = hck + T * nE;
    hipLaunchKernelGGL(k_gl_q0, dim3(gA), dim3(256), 0, h->stream, G, d_Q, qck);
    for (int t = 0; t < T; ++t) {
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, pas[t], G, d_x, feats, (const float *)(qck + (size_t)t * A), d_Q, dP, dR,
                           (float *)nullptr, (float *)nullptr);
        if (np > 0)
            hipLaunchKernelGGL(k_gl_epn_pair<0>, dim3(gP), w64, 0, h->stream, pas[t], L, (const float *)dP, (const float *)dR,
                               (const float *)nullptr, slotq, (float *)nullptr, (float *)nullptr, (float *)nullptr, GlTape{});
        hipLaunchKernelGGL(k_gl_epn_atom, dim3(gA), dim3(256), 0, h->stream, A, inc, (const float *)slotq, (const float *)(qck + (size_t)t * A),
                           qck + (size_t)(t + 1) * A);
    }
    HIPCHK(hipGetLastError());
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
            hipLaunchKernelGGL(k_gl_epn_pair<1>, dim3(gP), w64, 0, h->stream, pas[t], L, (const float *)dP, (const float *)dR,
                               (const float *)gq, (float *)nullptr, slotP, slotR, (float *)nullptr, K);
        hipLaunchKernelGGL(k_gl_epn_atom_bwd, dim3(A), w64, 0, h->stream, pas[t], G, inc, (const float *)slotP, (const float *)slotR, gh, gq, K);
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
        hipLaunchKernelGGL(k_gl_upd_bwd, dim3(A), w64, 0, h->stream, msg[t], upd, G, ht, (const float *)(Sck + t * nH), (const float *)gh,
                           ghp, dS, K);
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, msg[t], G, d_x, ht, (const float *)nullptr, d_Q, dP, dR, Yb, Yc);
        hipLaunchKernelGGL(k_tl_arow, dim3(gA64), dim3(256), 0, h->stream, G, d_x, ht, (const float *)nullptr, d_Q, arow);
        hipLaunchKernelGGL((k_gl_sweep<1, 1>), dim3(nw), w64, 0, h->stream, d_tasks, d_moff, A, msg[t].W2, (const float *)dP, (const float *)dR,
                           (const float *)Yb, (const float *)dS, partP, (int)nt, run, wpart);
        hipLaunchKernelGGL(k_gl_sweep<2>, dim3(nt), w64, 0, h->stream, d_tasks, d_moff, A, msg[t].W2, (const float *)dR, (const float *)dP,
                           (const float *)Yc, (const float *)dS, partR, (int)nt, 1, (float *)nullptr);
        const TDense *D = ts->msg[t];
        {                                                          // W2, b2 of all pairs: the sweep's partials
            TlRed Rs{};
            Rs.dst[0] = D[1].offW; Rs.len[0] = GL_H * GL_H; Rs.src[0] = 0;
            Rs.dst[1] = D[1].offB; Rs.len[1] = GL_H; Rs.src[1] = GL_H * GL_H;
            for (int k = 0; k < 2; ++k) { Rs.nblk[k] = (int)nw; Rs.stride[k] = GL_H * GL_H + GL_H; Rs.scale[k] = 1.f; }
            hipLaunchKernelGGL(k_tl_reduce, dim3(GL_H * GL_H / 64, 2), dim3(1024), 0, h->stream, Rs, (const float *)wpart, grad);
        }
        if (np > 0)
            hipLaunchKernelGGL(k_gl_gnn_pair<1>, dim3(gP), w64, 0, h->stream, msg[t], L, (const float *)dP, (const float *)dR,
                               (const float *)dS, slotP, slotR, (float *)nullptr, K);
        hipLaunchKernelGGL(k_gl_gnn_atom_bwd, dim3(A), w64, 0, h->stream, msg[t], G, inc, (const float *)partP, (const float *)partR,
                           (const float *)slotP, (const float *)slotR, (const float *)dP, (const float *)dS, ghp, K);
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
    if (B < 1 || N < 1 || offsets[0] != 0) EPNN_FAIL("%s: B and N must be positive and offsets[0] must be 0", name);
    for (int b = 0; b < B; ++b)
        if (offsets[b + 1] - offsets[b] > N || offsets[b + 1] - offsets[b] < 1) EPNN_FAIL("%s: molecule %d does not fit N=%d", name, b, N);
    std::vector<EpnnCell> cells;
    if (cell && check_cell(B, cell, (double)h->cfg.cutoff, name, cells)) return 1;
    if (!train_state(h)->ready) EPNN_FAIL("train step: call epnn_train_init first");
    // "train_path": 0 = by size, 1 = the dense path, 2 = the pair-list path (refused where it is not built)
    if (h->opt_train_path == 2 && h->upd_generic)
        EPNN_FAIL("%s: train_path = 2 (pair-list path) is built for update layers [32, 32] only (epnn_set_update_layers changed them)", name);
    if (h->opt_train_path == 2 && h->part_world != 1)
        EPNN_FAIL("%s: train_path = 2 (pair-list path) does not run on a partitioned handle (epnn_set_partition)", name);
    if (h->opt_train_path == 2 || (h->opt_train_path == 0 && grad_large_possible(h) && grad_large_auto(B, N))) {
        if (train_quiesce(h)) return 1;                          // a dense "train_async" step may still be reading the masters' gradients
        return train_step_large_impl(h, B, N, offsets, xyz, x, Q, cell ? cells.data() : nullptr, y_flat, q_out_flat, loss_out, apply);
    }
    return train_step_xyz_impl(h, B, N, offsets, xyz, x, Q, y_flat, q_out_flat, loss_out, apply, cell ? cells.data() : nullptr);
}
extern "C" int epnn_train_step_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                        const float *Q, const float *cell, const float *y_flat, float *q_out_flat, float *loss_out,
                                        int apply) {
    if (!train_step_guarded(h, apply)) return train_step_xyz_cell_impl(h, B, N, offsets, xyz, x, Q, cell, y_flat, q_out_flat, loss_out, apply);
    h->guard_pending = true;
    return comm_guard_exit(h, train_step_xyz_cell_impl(h, B, N, offsets, xyz, x, Q, cell, y_flat, q_out_flat, loss_out, apply),
                           "train step (gradient all-reduce)");
}
