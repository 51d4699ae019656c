// epnn_charges_vjp_xyz: charges and g^T dq/dxyz of a flat coordinate batch (kernels: epnn_grad_xyz.hip.h).
// Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_api_pairlist.hip.h"

// The call's own TrainState: the handle's current weights as a flat vector (refreshed when weights_gen moves on) and the
// scratch of one forward + backward.  The training state (masters, gradients, Adam moments, step) is never read or written.
static TrainState *xyz_grad_state(epnn_handle *h) {
    if (!h->xyz_grad) h->xyz_grad = new TrainState();
    return reinterpret_cast<TrainState *>(h->xyz_grad);
}
static void xyz_grad_release(epnn_handle *h) {
    if (!h->xyz_grad) return;
    TrainState *xs = reinterpret_cast<TrainState *>(h->xyz_grad);
    for (DevBuf *b : {&xs->theta, &xs->grad, &xs->m, &xs->v, &xs->part, &xs->arena, &xs->loss, &xs->d_step}) b->release();
    delete xs;
    h->xyz_grad = nullptr;
}

// ------------------------------------------------------------------------------------------------ pair-list path ("grad_path")
// State, weights, the call's set-up and the checkpointed forward: epnn_api_pairlist.hip.h.  Here: the reverse-mode entries' scratch and
// their one backward, for K cotangents (kernels: epnn_vjp_multi.hip.h; the single-cotangent entries are K = 1).
// One call of a reverse-mode entry, in the two pieces its entries share: gl_grad_forward (set-up, scratch, checkpointed forward) and
// gl_grad_backward (the backward from K seeds already on the device, in r.gq).  Between the two an entry writes its seeds.
struct GlGrad {
    GlCall c;
    size_t o_slotx, o_share, o_more[3];                          // o_more: the entry's own buffers, placed behind the shared ones
    float *hck, *Sck, *qck, *dP, *dR, *Yb, *Yc, *dS, *partP, *partR, *slotP, *slotR, *slotq, *gE, *gh, *ghp;
    float *out, *gq, *q_fin, *gx, *gs;                           // out: [K][A] gq | [A] q | [K][A][3] gxyz | bad | [K][B][9] gstrain
    int *bad;
};

// K: the cotangents; the backward's rows (dS, partP, partR, slotP, slotR, gE, gh, ghp, slotx, share, out) are K copies of one
// cotangent's, cotangent t at t times that size (the forward uses the first copy of partP and slotP as its scratch).
// spans: the entry's own staged inputs (r.c.d_extra); more[k] bytes: buffers of the entry alone (r.o_more[k]; the first one follows
// `out` directly); in_cap: epnn_last_stats counts the staged inputs with their buffer's capacity, not with this call's bytes.
static int gl_grad_forward(epnn_handle *h, GradLarge *gl, const char *where, int B, int N, const int32_t *offsets, const float *xyz,
                           const float *x, const float *Q, const HostGeo &geo, int K, const GlSpan *spans, int n_spans, const size_t *more,
                           int n_more, bool in_cap, GlGrad &r) {
    const int T = h->cfg.T, A = offsets[B];
    GlCall &c = r.c;
    if (gl_call_count(h, gl, where, B, N, offsets, xyz, x, Q, geo, spans, n_spans, c)) return 1;
    const size_t Kz = (size_t)K, P1 = c.P1, SL = 2 * P1, rowH = (size_t)A * GL_H * 4, rowE = (size_t)A * GL_E * 4, maxp = (size_t)c.maxp;
    const size_t o_h = c.place((size_t)(T + 1) * rowE), o_S = c.place((size_t)T * rowH),
                 o_q = c.place((size_t)(T + 1) * A * 4), o_P = c.place(rowH), o_R = c.place(rowH), o_Yb = c.place(rowH), o_Yc = c.place(rowH),
                 o_dS = c.place(Kz * rowH), o_partP = c.place(Kz * maxp * rowH), o_partR = c.place(Kz * maxp * rowH),
                 o_slotP = c.place(Kz * SL * GL_H * 4), o_slotR = c.place(Kz * SL * GL_H * 4), o_slotq = c.place(SL * 4),
                 o_gE = c.place(Kz * P1 * GL_E * 4), o_gh = c.place(Kz * rowE), o_ghp = c.place(Kz * rowE), o_slotx = c.place(Kz * SL * 72),
                 o_share = c.place(Kz * A * 48), o_out = c.place(((size_t)A + Kz * ((size_t)A * 4 + (size_t)B * 9) + 1) * 4);
    for (int k = 0; k < n_more; ++k) r.o_more[k] = c.place(more[k]);
    if (gl_call_fill(h, gl, c, in_cap ? gl->in.cap : c.in_total)) return 1;
    r.o_slotx = o_slotx; r.o_share = o_share;
    r.hck = c.fp(o_h); r.Sck = c.fp(o_S); r.qck = c.fp(o_q); r.dP = c.fp(o_P); r.dR = c.fp(o_R); r.Yb = c.fp(o_Yb); r.Yc = c.fp(o_Yc);
    r.dS = c.fp(o_dS); r.partP = c.fp(o_partP); r.partR = c.fp(o_partR); r.slotP = c.fp(o_slotP); r.slotR = c.fp(o_slotR);
    r.slotq = c.fp(o_slotq); r.gE = c.fp(o_gE); r.gh = c.fp(o_gh); r.ghp = c.fp(o_ghp); r.out = c.fp(o_out);
    r.gq = r.out;
    r.q_fin = r.out + Kz * A; r.gx = r.q_fin + A;
    r.bad = reinterpret_cast<int *>(r.gx + Kz * A * 3);
    r.gs = r.gx + Kz * A * 3 + 1;
    return gl_forward_ckpt(h, c, gl->msg, gl->pas, gl->upd, r.hck, r.Sck, r.qck, r.dP, r.dR, r.Yb, r.Yc, r.partP, r.slotP, r.slotq);
}

// A backward sweep over K cotangents in chunks, the widest instantiated k_gl_sweep<MODE, KC> that fits what is left (jvm_chunk: K = 7
// runs 4 + 2 + 1, K = 1 the one-row kernel).  dS, out: the first cotangent's, the next at dstride / ostride floats.
template <int MODE>
static void gvm_sweep_launch(epnn_handle *h, const GlCall &c, int K, const float *W2, const float *Xres, const float *Xstr, const float *Y,
                             const float *dS, size_t dstride, float *out, size_t ostride) {
    for (int k0 = 0; k0 < K;) {
        const int kc = jvm_chunk(K - k0);
        const float *cd = dS + k0 * dstride;
        float *co = out + k0 * ostride;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(c.nt), dim3(64), 0, h->stream, c.d_tasks, c.d_moff, c.G.A, W2, Xres, Xstr, Y, cd, dstride, co, ostride,
                               (int)c.nt, 1, (float *)nullptr);
        };
        if (kc == 4) launch(k_gl_sweep<MODE, 4>);
        else if (kc == 2) launch(k_gl_sweep<MODE, 2>);
        else launch(k_gl_sweep<MODE, 1>);
        k0 += kc;
    }
}

// The listed pairs' edge gradients gE [K][P1][48] -> their coordinate slots, in the call's geometry (box rows: K = 1 only, the multi
// entry takes cells)
template <int KM>
static void launch_gvm_pair_xyz(epnn_handle *h, const GlCall &c, int K, const float *gE, double *slotx, int *bad) {
    geo_dispatch(c.geo.kind, [&](auto kind) {
        if constexpr (decltype(kind)::value != GEO_BOX || KM == 1)
            hipLaunchKernelGGL((k_gvm_pair_xyz<decltype(kind)::value, KM>), dim3((unsigned)((c.np + 255) / 256)), dim3(256), 0, h->stream, c.L, c.np,
                               K, c.P1, 2 * c.P1, c.d_molof, c.d_xyz, c.geo.words(), gE, (double)h->cfg.cutoff, (double)h->cfg.eta,
                               h->d_mu.as<double>(), slotx, bad);
    });
}

// The backward from the K seeds in r.gq (overwritten), down to gxyz (r.gx), the strain derivative (r.gs; want_strain) and the final
// charges beside them (r.q_fin): everything up to the entry's download.  The per-pair and per-atom kernels are chosen by the bucket
// of K (jvm_bucket).
static int gl_grad_backward(epnn_handle *h, GradLarge *gl, GlGrad &r, int B, int K, bool want_strain) {
    const GlCall &c = r.c;
    if (c.geo.kind == GEO_BOX && K > 1) EPNN_FAIL("gl_grad_backward: internal error (box rows with K = %d: the coordinate kernel takes them at K = 1 only)", K);
    const int T = h->cfg.T, A = c.G.A, np = c.np;
    const size_t Kz = (size_t)K, P1 = c.P1, SL = 2 * P1;
    const unsigned gP = (unsigned)np, gA = c.gA;
    const GlGeom &G = c.G;
    const GlPairs &L = c.L;
    const int *inc = c.inc;
    const float *d_x = c.d_x, *d_Q = c.d_Q;
    float *hck = r.hck, *Sck = r.Sck, *qck = r.qck, *dP = r.dP, *dR = r.dR, *Yb = r.Yb, *Yc = r.Yc, *dS = r.dS, *partP = r.partP,
          *partR = r.partR, *slotP = r.slotP, *slotR = r.slotR, *gE = r.gE, *gh = r.gh, *ghp = r.ghp, *gq = r.gq, *gx = r.gx, *gs = r.gs;
    int *bad = r.bad;
    const size_t nH = (size_t)A * GL_H, nE = (size_t)A * GL_E, pstride = (size_t)c.maxp * nH;
    const dim3 w64(64);
    const float *feats = hck + T * nE;
    // ---- backward: EPN stack
    HIPCHK(hipMemsetAsync(gh, 0, Kz * nE * 4, h->stream));
    HIPCHK(hipMemsetAsync(gE, 0, Kz * P1 * GL_E * 4, h->stream));
    HIPCHK(hipMemsetAsync(bad, 0, 4, h->stream));
    for (int t = T - 1; t >= 0; --t) {
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, gl->pas[t], G, d_x, feats, (const float *)(qck + (size_t)t * A), d_Q, dP, dR,
                           (float *)nullptr, (float *)nullptr);
        if (np > 0)
            jvm_bucket(K, [&](auto km) {
                hipLaunchKernelGGL((k_gvm_epn_pair<decltype(km)::value>), dim3(gP), w64, 0, h->stream, gl->pas[t], L, K, A, P1, SL, (const float *)dP,
                                   (const float *)dR, (const float *)gq, slotP, slotR, gE, GlTape{});
            });
        jvm_bucket(K, [&](auto km) {
            hipLaunchKernelGGL((k_gvm_epn_atom_bwd<decltype(km)::value>), dim3(A), w64, 0, h->stream, gl->pas[t], G, K, SL, inc, (const float *)slotP,
                               (const float *)slotR, gh, gq, GlTape{});
        });
    }
    HIPCHK(hipGetLastError());
    // ---- backward: GNN steps
    for (int t = T - 1; t >= 0; --t) {
        const float *ht = t ? hck + t * nE : nullptr;
        jvm_bucket(K, [&](auto km) {
            hipLaunchKernelGGL((k_gvm_upd_bwd<decltype(km)::value>), dim3(A), w64, 0, h->stream, gl->msg[t], gl->upd, G, K, ht,
                               (const float *)(Sck + t * nH), (const float *)gh, ghp, dS, GlTape{});
        });
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, gl->msg[t], G, d_x, ht, (const float *)nullptr, d_Q, dP, dR, Yb, Yc);
        if (t == 0) {                                            // a_i of step 0 is constant: only dG of the listed pairs
            if (np > 0)
                jvm_bucket(K, [&](auto km) {
                    hipLaunchKernelGGL((k_gvm_gnn_pair<decltype(km)::value>), dim3(gP), w64, 0, h->stream, gl->msg[t], L, K, A, P1, SL,
                                       (const float *)dP, (const float *)dR, (const float *)dS, (float *)nullptr, (float *)nullptr, gE, GlTape{});
                });
            break;
        }
        gvm_sweep_launch<1>(h, c, K, gl->msg[t].W2, dP, dR, Yb, dS, nH, partP, pstride);
        gvm_sweep_launch<2>(h, c, K, gl->msg[t].W2, dR, dP, Yc, dS, nH, partR, pstride);
        if (np > 0)
            jvm_bucket(K, [&](auto km) {
                hipLaunchKernelGGL((k_gvm_gnn_pair<decltype(km)::value>), dim3(gP), w64, 0, h->stream, gl->msg[t], L, K, A, P1, SL, (const float *)dP,
                                   (const float *)dR, (const float *)dS, slotP, slotR, gE, GlTape{});
            });
        jvm_bucket(K, [&](auto km) {
            hipLaunchKernelGGL((k_gvm_gnn_atom_bwd<decltype(km)::value>), dim3(A), w64, 0, h->stream, gl->msg[t], G, K, pstride, SL, inc,
                               (const float *)partP, (const float *)partR, (const float *)slotP, (const float *)slotR, (const float *)dP,
                               (const float *)dS, ghp, GlTape{});
        });
        std::swap(gh, ghp);
    }
    HIPCHK(hipGetLastError());
    // ---- edges -> coordinates
    double *slotx = reinterpret_cast<double *>(c.dw + r.o_slotx), *share = want_strain ? reinterpret_cast<double *>(c.dw + r.o_share) : nullptr;
    if (np > 0) jvm_bucket(K, [&](auto km) { launch_gvm_pair_xyz<decltype(km)::value>(h, c, K, gE, slotx, bad); });
    hipLaunchKernelGGL(k_gvm_atom_xyz, dim3(gA, (unsigned)K), dim3(256), 0, h->stream, A, SL, inc, (const double *)slotx, gx, share);
    if (share) hipLaunchKernelGGL(k_gvm_strain_mol, dim3((unsigned)B, (unsigned)K), dim3(64), 0, h->stream, A, (const double *)share, c.d_moff, gs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(r.q_fin, qck + (size_t)T * A, (size_t)A * 4, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// one cotangent: the single VJP and the Coulomb entries
static int gl_grad_backward(epnn_handle *h, GradLarge *gl, GlGrad &r, int B, bool want_strain) { return gl_grad_backward(h, gl, r, B, 1, want_strain); }

static int charges_vjp_large_impl(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                  const float *g, float *q_out, float *gxyz_out, const HostGeo &geo, float *gstrain_out) {
    GradLarge *gl = grad_large_state(h);
    if (grad_large_weights(h, gl)) return 1;
    const int A = offsets[B];
    const std::string where = std::string(name) + " (pair-list path)";
    const GlSpan span_g{g, (size_t)A * 4, false};
    GlGrad r;
    if (gl_grad_forward(h, gl, where.c_str(), B, N, offsets, xyz, x, Q, geo, 1, &span_g, 1, nullptr, 0, true, r)) return 1;
    HIPCHK(hipMemcpyAsync(r.gq, r.c.d_extra[0], (size_t)A * 4, hipMemcpyDeviceToDevice, h->stream));    // the seed: the staged g
    if (gl_grad_backward(h, gl, r, B, gstrain_out != nullptr)) return 1;
    const float *q_fin = r.q_fin;
    const size_t nback = (size_t)A * 4 + 1 + (gstrain_out ? (size_t)B * 9 : 0);
    if (gl->pin_out.ensure(nback * 4)) return 1;
    float *back = gl->pin_out.as<float>();
    HIPCHK(hipMemcpyAsync(back, q_fin, nback * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (reinterpret_cast<const int *>(back)[4 * (size_t)A] & 2) EPNN_FAIL("%s (pair-list path): the pair list is not symmetric", name);
    if (reinterpret_cast<const int *>(back)[4 * (size_t)A] != 0)
        EPNN_FAIL("%s: two atoms of a molecule%s coincide (distance 0: the edge features have no derivative there)", name,
                  geo.periodic() ? " or their periodic images" : "");
    memcpy(q_out, back, (size_t)A * 4);
    memcpy(gxyz_out, back + A, (size_t)A * 12);
    if (gstrain_out) memcpy(gstrain_out, back + 4 * (size_t)A + 1, (size_t)B * 9 * 4);
    return 0;
}

// the edge gradients gE [B][N][N][48] -> gxyz, a wavefront per atom, in the call's geometry; share: with cells, the atoms' strain shares, or null
static void launch_g_xyz(epnn_handle *h, int A, const float *d_xyz, const int *d_moff, int B, int N, const float *gE, float *gxyz, int *bad,
                         const DevGeo &geo, double *share) {
    geo_dispatch(geo.kind, [&](auto kind) {
        hipLaunchKernelGGL(k_g_xyz<decltype(kind)::value>, dim3((unsigned)A), dim3(64), 0, h->stream, d_xyz, d_moff, B, N, gE,
                           (double)h->cfg.cutoff, (double)h->cfg.eta, h->d_mu.as<double>(), gxyz, bad, geo.words(), share);
    });
}

// name: the entry's; geo: the batch's geometry, its rows on the host (staged with the other inputs); gstrain_out [B][3][3]:
// with cells, the strain derivative (k_g_xyz<GEO_CELL> / k_g_strain_mol), or null.
static int charges_vjp_xyz_impl(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                const float *g, float *q_out, float *gxyz_out, const HostGeo &geo, float *gstrain_out) {
    for (int b = 0; b < B; ++b)
        if (offsets[b + 1] - offsets[b] > N || offsets[b + 1] - offsets[b] < 1) EPNN_FAIL("epnn_charges_vjp_xyz: molecule %d does not fit N=%d", b, N);
    EPNN_NOT_FUSED_ONLY(h, "epnn_charges_vjp_xyz");
    HIPCHK(hipSetDevice(h->device));
    if (h->pending.active && finish_forward(h)) return 1;
    // the weights epnn_forward_xyz would use: a training step still in flight is waited for, device masters it has updated are
    // pulled into the host copies (pack_weights; what any inference call does first)
    if (train_quiesce(h) || pack_weights(h)) return 1;
    // "grad_path": 0 = by size, 1 = the dense path below, 2 = the pair-list path (refused where it is not built)
    if (h->opt_grad_path == 2 && h->upd_generic)
        EPNN_FAIL("epnn_charges_vjp_xyz: grad_path = 2 (pair-list path) is built for update layers [32, 32] only (epnn_set_update_layers changed them)");
    if (h->opt_grad_path == 2 && h->part_world != 1)
        EPNN_FAIL("epnn_charges_vjp_xyz: grad_path = 2 (pair-list path) does not run on a partitioned handle (epnn_set_partition)");
    if (h->opt_grad_path == 2 || (h->opt_grad_path == 0 && grad_large_possible(h) && grad_large_auto(B, N)))
        return charges_vjp_large_impl(h, name, B, N, offsets, xyz, x, Q, g, q_out, gxyz_out, geo, gstrain_out);
    TrainState *xs = xyz_grad_state(h);
    if (!xs->ready || xs->step != h->weights_gen) {
        train_layout(h, xs);
        if (xs->theta.ensure((size_t)xs->P * 4)) return 1;
        std::vector<float> flat;
        train_gather_host(h, xs, flat);
        HIPCHK(hipMemcpyAsync(xs->theta.p, flat.data(), (size_t)xs->P * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));               // (`flat` is pageable and goes out of scope)
        xs->step = h->weights_gen;                              // (this state takes no optimizer steps: `step` keeps the generation)
        xs->ready = true;
    }
    const int A = offsets[B];
    // the train path's inputs, staged and padded as epnn_train_step_xyz does (dense_in_stage); the label slot carries -g / 2 (see XyzGrad)
    const DenseIn L(h, B, N, A, geo);
    const size_t pairs = L.pairs, slots = L.slots;
    if (dense_in_ensure(h, L)) return 1;
    // [BN] loss terms | [BN] predictions | [BN] zeros | [A][3] gxyz | the coincident-atoms flag;  gE [R][48]
    // ... | [B][9] gstrain (when asked for); behind them, not downloaded, the atoms' strain shares [A][6] float64
    const size_t o_zero = 2 * slots, o_gx = 3 * slots, o_bad = o_gx + (size_t)A * 3, o_gs = o_bad + 1,
                 nout = o_gs + (gstrain_out ? (size_t)B * 9 : 0), o_share = (nout * 4 + 7) & ~size_t(7);
    if (xs->loss.ensure(gstrain_out ? o_share + (size_t)A * 48 : nout * 4) || xs->grad.ensure(pairs * 48 * 4)) return 1;
    if (dense_in_stage(h, L, B, N, offsets, xyz, x, Q, geo, [&](float *ys) { for (int a = 0; a < A; ++a) ys[a] = -0.5f * g[a]; })) return 1;
    HIPCHK(hipGetLastError());
    const int *d_moff = h->s_train.as<int>();
    float *out = xs->loss.as<float>();
    HIPCHK(hipMemsetAsync(out + o_zero, 0, (slots + (size_t)A * 3 + 1) * 4, h->stream));
    HIPCHK(hipMemsetAsync(xs->grad.p, 0, pairs * 48 * 4, h->stream));
    XyzGrad xg{xs, h->sd_out.as<float>(), out + o_zero, xs->grad.as<float>(), h->tr_realbuf.as<int>()};
    // the padded slots are exact zeros in every input, as in a coordinate train step: the matrix-pipe kernels skip them
    if (h->opt_train_skip_padded) { h->tr_moff = d_moff; h->tr_real = h->tr_realbuf.as<int>(); }
    int rc;
    if (train_is_fused(h, N))
        rc = train_fwd_bwd_fused(h, B, N, h->sd_e.as<float>(), h->sd_mask.as<float>(), h->dn_xs.as<float>(), h->dn_hs.as<float>(),
                                 h->dn_qs.as<float>(), h->sd_out.as<float>(), out + slots, out, false, false, nullptr, false, &xg);
    else
        rc = train_fwd_bwd(h, B, N, h->sd_e.as<float>(), h->sd_mask.as<float>(), h->dn_xs.as<float>(), h->dn_hs.as<float>(),
                           h->dn_qs.as<float>(), h->sd_out.as<float>(), out + slots, out, false, &xg);
    h->tr_moff = nullptr;
    h->tr_real = nullptr;
    if (rc) return 1;
    double *share = gstrain_out && geo.kind == GEO_CELL ? reinterpret_cast<double *>(xs->loss.as<char>() + o_share) : nullptr;
    launch_g_xyz(h, A, reinterpret_cast<const float *>(h->s_train.as<char>() + L.o_xyz), d_moff, B, N, xs->grad.as<float>(), out + o_gx,
                 reinterpret_cast<int *>(out + o_bad), geo_on_device(geo, h->s_train.as<char>() + L.o_geo), share);
    if (share) hipLaunchKernelGGL(k_g_strain_mol, dim3((unsigned)B), dim3(64), 0, h->stream, share, d_moff, out + o_gs);
    HIPCHK(hipGetLastError());
    // predictions | zeros | gxyz | flag: one download
    if (h->pin_tout.ensure((nout - slots) * 4)) return 1;
    float *back = h->pin_tout.as<float>();
    HIPCHK(hipMemcpyAsync(back, out + slots, (nout - slots) * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (reinterpret_cast<const int *>(back)[o_bad - slots] != 0)
        EPNN_FAIL("%s: two atoms of a molecule%s coincide (distance 0: the edge features have no derivative there)", name,
                  geo.periodic() ? " or their periodic images" : "");
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < offsets[b + 1] - offsets[b]; ++i) q_out[offsets[b] + i] = back[(size_t)b * N + i];
    memcpy(gxyz_out, back + (o_gx - slots), (size_t)A * 3 * 4);
    if (gstrain_out) memcpy(gstrain_out, back + (o_gs - slots), (size_t)B * 9 * 4);
    return 0;
}

extern "C" int epnn_charges_vjp_xyz(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                    const float *Q, const float *g, float *q_out, float *gxyz_out) {
    if (!h || !offsets || !xyz || !x || !Q || !g || !q_out || !gxyz_out) EPNN_FAIL("epnn_charges_vjp_xyz: null argument");
    if (B < 1 || N < 1 || offsets[0] != 0) EPNN_FAIL("epnn_charges_vjp_xyz: B and N must be positive and offsets[0] must be 0");
    return charges_vjp_xyz_impl(h, "epnn_charges_vjp_xyz", B, N, offsets, xyz, x, Q, g, q_out, gxyz_out, HostGeo{}, nullptr);
}

extern "C" int epnn_charges_vjp_xyz_pbc(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                        const float *Q, const float *box, const float *g, float *q_out, float *gxyz_out) {
    if (!h || !offsets || !xyz || !x || !Q || !g || !q_out || !gxyz_out) EPNN_FAIL("epnn_charges_vjp_xyz_pbc: null argument");
    if (B < 1 || N < 1 || offsets[0] != 0) EPNN_FAIL("epnn_charges_vjp_xyz_pbc: B and N must be positive and offsets[0] must be 0");
    GeoArg arg;
    if (arg.box(B, box, (double)h->cfg.cutoff, "epnn_charges_vjp_xyz_pbc")) return 1;
    return charges_vjp_xyz_impl(h, "epnn_charges_vjp_xyz_pbc", B, N, offsets, xyz, x, Q, g, q_out, gxyz_out, arg.geo, nullptr);
}

extern "C" int epnn_charges_vjp_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                         const float *Q, const float *cell, const float *g, float *q_out, float *gxyz_out,
                                         float *gstrain_out) {
    if (!h || !offsets || !xyz || !x || !Q || !g || !q_out || !gxyz_out) EPNN_FAIL("epnn_charges_vjp_xyz_cell: null argument");
    if (B < 1 || N < 1 || offsets[0] != 0) EPNN_FAIL("epnn_charges_vjp_xyz_cell: B and N must be positive and offsets[0] must be 0");
    GeoArg arg;
    if (arg.cell(B, cell, (double)h->cfg.cutoff, "epnn_charges_vjp_xyz_cell")) return 1;
    return charges_vjp_xyz_impl(h, "epnn_charges_vjp_xyz_cell", B, N, offsets, xyz, x, Q, g, q_out, gxyz_out, arg.geo, gstrain_out);
}
