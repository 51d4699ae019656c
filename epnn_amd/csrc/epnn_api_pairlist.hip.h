// What the pair-list entries share on the host: the state GradLarge, their weights, one call's set-up (GlCall: staged inputs, the
// front-end's pair list, the work buffer) and the checkpointed forward of the two reverse-mode entries.  Entries:
// charges_vjp_large_impl (epnn_api_grad.hip.h, "grad_path"), train_step_large_impl (epnn_api_train_large.hip.h, "train_path"),
// charges_jvp_multi_impl (epnn_api_jvp.hip.h), coulomb_run (epnn_api_coulomb_run.hip.h, through the gradient call's two pieces).  Host code only; kernels: epnn_frontend.hip.h, epnn_grad_large.hip.h
// (forward, sweep), epnn_vjp_multi.hip.h (backward).
// Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_grad_large.hip.h"
#include "epnn_vjp_multi.hip.h"

// ------------------------------------------------------------------------------------------------ pair-list path ("grad_path")
// The same result from the pair list (kernels and arithmetic: epnn_grad_large.hip.h): per-atom rows, the near pairs of the
// separate front-end and their incidence slots, nothing of size N^2.  Its own weights (plain Keras layout, refreshed when
// weights_gen moves on), inputs and scratch: neither the training state nor the forward's plan and pair list are touched.
struct GradLarge {
    long wgen = -1;
    DevBuf w, in, work;
    PinBuf pin_in, pin_out;
    GlPair msg[EPNN_MAXT], pas[EPNN_MAXT];
    GlUpd upd;
};
static GradLarge *grad_large_state(epnn_handle *h) {
    if (!h->grad_large) h->grad_large = new GradLarge();
    return reinterpret_cast<GradLarge *>(h->grad_large);
}
static void grad_large_release(epnn_handle *h) {
    if (!h->grad_large) return;
    GradLarge *gl = reinterpret_cast<GradLarge *>(h->grad_large);
    gl->w.release(); gl->in.release(); gl->work.release(); gl->pin_in.release(); gl->pin_out.release();
    delete gl;
    h->grad_large = nullptr;
}
static bool grad_large_possible(const epnn_handle *h) { return !h->upd_generic && h->part_world == 1; }
// automatic routing: the dense path while its [B][N][N] tensors stay small (no caller of this repository's tests, bench or tools
// is above it, so every call that ran before takes the path it took)
static bool grad_large_auto(int B, int N) { return (size_t)B * (size_t)N * (size_t)N > ((size_t)1 << 22); }

// ------------------------------------------------------------------------------------------------ K tangents or cotangents
// A sweep carries them in chunks: the widest instantiated kernel that fits what is left, so K = 7 runs 4 + 2 + 1.
static int jvm_chunk(int left) { return left >= 4 ? 4 : left >= 2 ? 2 : 1; }

// The per-pair and per-atom kernels are instantiated for buckets of K, KM = 1, 2, 4, 8, 16: launch(km) is called with the bucket
// as an integral constant.
template <class Launch>
static void jvm_bucket(int K, Launch &&launch) {
    if (K <= 1) launch(std::integral_constant<int, 1>{});
    else if (K <= 2) launch(std::integral_constant<int, 2>{});
    else if (K <= 4) launch(std::integral_constant<int, 4>{});
    else if (K <= 8) launch(std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 16>{});
}

// ------------------------------------------------------------------------------------------------ weights
// Dense: HostDense (the handle's host copies) or TDense (the training state's flat vector); F = nx + 48 + 1 input features per atom
template <class Dense>
static int gl_check_shapes(const char *entry, int T, int F, const Dense (*msg)[3], const Dense (*pas)[3], const Dense *upd) {
    for (int t = 0; t < T; ++t)
        for (int pass = 0; pass < 2; ++pass) {
            const Dense *L = pass ? pas[t] : msg[t];
            if (L[0].n_in != 2 * F + GL_E || L[0].n_out != GL_H || L[1].n_in != GL_H || L[1].n_out != GL_H || L[2].n_in != GL_H ||
                L[2].n_out != (pass ? 1 : GL_H))
                EPNN_FAIL("%s (pair-list path): unexpected shape of a %s MLP", entry, pass ? "pass" : "message");
        }
    if (upd[0].n_in != GL_E + GL_H || upd[0].n_out != GL_H || upd[1].n_out != GL_H || upd[2].n_out != GL_E)
        EPNN_FAIL("%s (pair-list path): unexpected shape of the update MLP", entry);
    return 0;
}
// a message / pass MLP inside a flat vector: the first Dense's kernel is the blocks Wi | Wj | We
static void gl_point_pair(GlPair &M, const float *base, size_t offW0, size_t offB0, size_t offW1, size_t offB1, size_t offW2, size_t offB2,
                          int F) {
    M.Wi = base + offW0; M.Wj = M.Wi + (size_t)F * GL_H; M.We = M.Wj + (size_t)F * GL_H;
    M.b1 = base + offB0; M.W2 = base + offW1; M.b2 = base + offB1; M.W3 = base + offW2; M.b3 = base + offB2;
}

static int grad_large_weights(epnn_handle *h, GradLarge *gl) {
    if (gl->wgen == h->weights_gen) return 0;
    const int F = h->cfg.nx + GL_E + 1, T = h->cfg.T;
    if (gl_check_shapes("epnn_charges_vjp_xyz", T, F, h->msg, h->pas, h->upd)) return 1;
    std::vector<float> flat;
    auto put = [&](const std::vector<float> &v) { const size_t o = flat.size(); flat.insert(flat.end(), v.begin(), v.end()); return o; };
    size_t om[EPNN_MAXT][6], op[EPNN_MAXT][6], ou[6];
    for (int t = 0; t < T; ++t)
        for (int pass = 0; pass < 2; ++pass)
            for (int l = 0; l < 3; ++l) {
                const HostDense &D = pass ? h->pas[t][l] : h->msg[t][l];
                (pass ? op[t] : om[t])[2 * l] = put(D.W);
                (pass ? op[t] : om[t])[2 * l + 1] = put(D.b);
            }
    for (int l = 0; l < 3; ++l) { ou[2 * l] = put(h->upd[l].W); ou[2 * l + 1] = put(h->upd[l].b); }
    HIPCHK(hipStreamSynchronize(h->stream));                      // (no call of this path is in flight: they all end with a wait)
    if (gl->w.ensure(flat.size() * 4)) return 1;
    if (copy_sync(h, gl->w.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice)) return 1;
    const float *base = gl->w.as<float>();
    for (int t = 0; t < T; ++t) {
        gl_point_pair(gl->msg[t], base, om[t][0], om[t][1], om[t][2], om[t][3], om[t][4], om[t][5], F);
        gl_point_pair(gl->pas[t], base, op[t][0], op[t][1], op[t][2], op[t][3], op[t][4], op[t][5], F);
    }
    gl->upd = GlUpd{base + ou[0], base + ou[1], base + ou[2], base + ou[3], base + ou[4], base + ou[5]};
    gl->wgen = h->weights_gen;
    return 0;
}

// ------------------------------------------------------------------------------------------------ one call's set-up
// an input of one entry alone, staged behind Q: `bytes` from src; src null: zeros if `zero`, else not written
struct GlSpan { const void *src; size_t bytes; bool zero; };
struct GlCall {
    const int *d_moff, *d_molof;  // the staged inputs, on the device
    const int4 *d_tasks;          // sweep tasks: 16 resident atoms x one piece of their molecule's partner range
    const float *d_xyz, *d_x, *d_Q, *d_extra[3];      // d_extra[k]: span k, null if it is empty
    DevGeo geo;                   // the call's geometry, its rows staged behind the spans
    FrontArgs F;
    GlGeom G;
    GlPairs L;
    const int *inc;               // [A + 1] incidence rows
    unsigned nt, gA;              // tasks; grid of one thread per atom
    int maxp, np;                 // most pieces of a partner range; listed pairs
    size_t P1;                    // max(np, 1)
    size_t in_total;              // bytes of the input block with the front-end's counts
    size_t o_pair[10];            // the pair list at the front of the work buffer; the entry's scratch follows: place()
    size_t at;                    // work-buffer cursor
    char *dw;                     // work buffer (gl_call_fill)
    size_t place(size_t bytes) { const size_t o = at; at += (bytes + 255) & ~size_t(255); return o; }      // 256-byte steps
    float *fp(size_t o) const { return reinterpret_cast<float *>(dw + o); }
};

// Stages the inputs (one upload), counts the pairs and checks the counts; `where` opens the two failure texts.  Afterwards the
// entry places its scratch behind the pair list (c.place) and calls gl_call_fill.
static int gl_call_count(epnn_handle *h, GradLarge *gl, const char *where, int B, int N, const int32_t *offsets, const float *xyz,
                         const float *x, const float *Q, const HostGeo &geo, const GlSpan *extras, int n_extras, GlCall &c) {
    const int nx = h->cfg.nx, A = offsets[B];
    std::vector<int4> tasks;
    c.maxp = 1;
    for (int b = 0; b < B; ++b) {
        const int n = offsets[b + 1] - offsets[b], np = gl_pieces(n);
        c.maxp = std::max(c.maxp, np);
        for (int a0 = offsets[b]; a0 < offsets[b + 1]; a0 += 16)
            for (int k = 0; k < np; ++k) tasks.push_back(make_int4(a0, b, k, np));
    }
    c.nt = (unsigned)tasks.size();
    // ---- inputs and the front-end's per-atom counts: one upload
    c.at = 0;
    const size_t o_off = c.place((size_t)(B + 1) * 4), o_molof = c.place((size_t)A * 4), o_mflag = c.place((size_t)B * 4),
                 o_task = c.place(tasks.size() * sizeof(int4)), o_xyz = c.place((size_t)A * 12), o_x = c.place((size_t)A * nx * 4),
                 o_Q = c.place((size_t)B * 4);
    size_t o_extra[3] = {0, 0, 0};
    for (int k = 0; k < n_extras; ++k) o_extra[k] = c.place(extras[k].bytes);
    const size_t o_geo = c.place(geo.bytes(B)), in_bytes = c.at;
    const size_t o_rowcnt = c.place((size_t)(A + 1) * 4), o_rowoff = c.place((size_t)(A + 1) * 4), o_deg = c.place((size_t)(A + 1) * 4),
                 o_incoff = c.place((size_t)(A + 1) * 4), o_status = c.place(16);
    c.in_total = c.at;
    if (gl->pin_in.ensure(in_bytes) || gl->in.ensure(c.in_total) || gl->pin_out.ensure(64)) return 1;
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
    for (int k = 0; k < n_extras; ++k) {
        if (extras[k].src) memcpy(st + o_extra[k], extras[k].src, extras[k].bytes);
        else if (extras[k].zero) memset(st + o_extra[k], 0, extras[k].bytes);
    }
    if (geo.periodic()) memcpy(st + o_geo, geo.rows, geo.bytes(B));
    char *din = gl->in.as<char>();
    HIPCHK(hipMemcpyAsync(din, st, in_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(din + o_status, 0, 16, h->stream));
    auto dfp = [&](size_t o) { return reinterpret_cast<const float *>(din + o); };
    auto dip = [&](size_t o) { return reinterpret_cast<int *>(din + o); };
    c.d_moff = dip(o_off); c.d_molof = dip(o_molof);
    c.d_tasks = reinterpret_cast<const int4 *>(din + o_task);
    c.d_xyz = dfp(o_xyz); c.d_x = dfp(o_x); c.d_Q = dfp(o_Q);
    c.geo = geo_on_device(geo, din + o_geo);
    for (int k = 0; k < 3; ++k) c.d_extra[k] = k < n_extras && extras[k].bytes ? dfp(o_extra[k]) : nullptr;
    // ---- pair list: count and prefix sums first, then buffers of exactly that size (gl_call_fill)
    FrontArgs &F = c.F;
    F = FrontArgs{};
    F.xyz = c.d_xyz; F.mol_of = c.d_molof; F.moff = c.d_moff; F.mflag = dip(o_mflag);
    F.A = A;
    F.cutoff = (double)h->cfg.cutoff; F.cut2 = cutoff_squared(F.cutoff); F.eta = (double)h->cfg.eta; F.tol = h->cfg.near_tol;
    F.e_dim = h->cfg.e_dim;
    F.mu = h->d_mu.as<double>();
    F.row_cnt = dip(o_rowcnt); F.row_off = dip(o_rowoff); F.deg = dip(o_deg); F.inc_off = dip(o_incoff); F.status = dip(o_status);
    F.pcap = 0x7fffffff;
    c.gA = (unsigned)((A + 255) / 256);
    launch_front_count(h, F, c.geo);
    HIPCHK(hipGetLastError());
    int *cnt = gl->pin_out.as<int>();
    HIPCHK(hipMemcpyAsync(cnt, F.row_off + A, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cnt + 1, F.inc_off + A, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cnt + 2, F.status, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    c.np = cnt[0];
    if (cnt[2] != 0) EPNN_FAIL("%s: the pair count overflowed (status %d)", where, cnt[2]);
    if (c.np < 0 || cnt[1] != 2 * c.np) EPNN_FAIL("%s: inconsistent pair count (%d pairs, %d incidences)", where, c.np, cnt[1]);
    c.P1 = (size_t)std::max(c.np, 1);
    c.G = GlGeom{c.d_moff, c.d_molof, A, N, nx};
    c.inc = F.inc_off;
    // pi, pj, psym, pe, pwi, pwj, nbr, dest_i, dest_j, prec
    const size_t P1 = c.P1, bytes[10] = {P1 * 4, P1 * 4, P1 * 4, P1 * GL_E * 4, P1 * 4, P1 * 4, 2 * P1 * 4, P1 * 4, P1 * 4,
                                         2 * (P1 + 256) * sizeof(int4)};
    c.at = 0;
    for (int k = 0; k < 10; ++k) c.o_pair[k] = c.place(bytes[k]);
    return 0;
}

// The work buffer of c.at bytes, the records of the listed pairs and their incidence slots.  stats[2], the device scratch of the
// call in bytes, is c.at + in_bytes: the reverse-mode entries pass the input buffer's capacity, the JVP c.in_total (they differ).
static int gl_call_fill(epnn_handle *h, GradLarge *gl, GlCall &c, size_t in_bytes) {
    if (gl->work.ensure(c.at)) return 1;
    h->stats[0] = c.np;
    h->stats[1] = 0;
    h->stats[3] = 0;
    h->stats[2] = (int64_t)(c.at + in_bytes);
    c.dw = gl->work.as<char>();
    auto ip = [&](int k) { return reinterpret_cast<int *>(c.dw + c.o_pair[k]); };
    FrontArgs &F = c.F;
    F.pcap = (int)c.P1;
    F.pi = ip(0); F.pj = ip(1); F.psym = ip(2); F.pe = c.fp(c.o_pair[3]); F.pwi = c.fp(c.o_pair[4]); F.pwj = c.fp(c.o_pair[5]);
    F.nbr = ip(6); F.dest_i = ip(7); F.dest_j = ip(8); F.prec = reinterpret_cast<int4 *>(c.dw + c.o_pair[9]);
    if (c.np > 0) {
        launch_front_fill(h, F, c.geo);             // (F.pcap is c.P1)
        HIPCHK(hipGetLastError());
    }
    c.L = GlPairs{F.pi, F.pj, F.dest_i, F.dest_j, F.pe, F.pwi};
    return 0;
}

// The forward of the reverse-mode entries with its checkpoints: hck [T + 1][A][48] (h_t; row 0 unused: h_0 = 0), Sck [T][A][32],
// qck [T + 1][A].  dP, dR, Yb, Yc [A][32], partP [maxp][A][32], slotP [2 P1][32] and slotq [2 P1] are scratch.
static int gl_forward_ckpt(epnn_handle *h, const GlCall &c, const GlPair *msg, const GlPair *pas, const GlUpd &upd, float *hck, float *Sck,
                           float *qck, float *dP, float *dR, float *Yb, float *Yc, float *partP, float *slotP, float *slotq) {
    const int T = h->cfg.T, A = c.G.A, np = c.np;
    const size_t nH = (size_t)A * GL_H, nE = (size_t)A * GL_E;
    const unsigned nt = c.nt, gP = (unsigned)np, gA = c.gA;
    const GlGeom &G = c.G;
    const GlPairs &L = c.L;
    const dim3 w64(64);
    for (int t = 0; t < T; ++t) {
        const float *ht = t ? hck + t * nE : nullptr;
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, msg[t], G, c.d_x, ht, (const float *)nullptr, c.d_Q, dP, dR, Yb, Yc);
        hipLaunchKernelGGL(k_gl_sweep<0>, dim3(nt), w64, 0, h->stream, c.d_tasks, c.d_moff, A, msg[t].W2, (const float *)dP, (const float *)dR,
                           (const float *)Yb, (const float *)nullptr, (size_t)0, partP, (size_t)0, (int)nt, 1, (float *)nullptr);
        if (np > 0)
            hipLaunchKernelGGL(k_gl_gnn_pair, dim3(gP), w64, 0, h->stream, msg[t], L, (const float *)dP, (const float *)dR, slotP);
        hipLaunchKernelGGL(k_gl_gnn_tail, dim3(A), w64, 0, h->stream, msg[t], upd, G, c.inc, (const float *)partP, (const float *)slotP,
                           (const float *)dP, ht, Sck + t * nH, hck + (t + 1) * nE);
    }
    HIPCHK(hipGetLastError());
    const float *feats = hck + T * nE;
    hipLaunchKernelGGL(k_gl_q0, dim3(gA), dim3(256), 0, h->stream, G, c.d_Q, qck);
    for (int t = 0; t < T; ++t) {
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, pas[t], G, c.d_x, feats, (const float *)(qck + (size_t)t * A), c.d_Q, dP, dR,
                           (float *)nullptr, (float *)nullptr);
        if (np > 0)
            hipLaunchKernelGGL(k_gl_epn_pair, dim3(gP), w64, 0, h->stream, pas[t], L, (const float *)dP, (const float *)dR, slotq);
        hipLaunchKernelGGL(k_gl_epn_atom, dim3(gA), dim3(256), 0, h->stream, A, c.inc, (const float *)slotq, (const float *)(qck + (size_t)t * A),
                           qck + (size_t)(t + 1) * A);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
