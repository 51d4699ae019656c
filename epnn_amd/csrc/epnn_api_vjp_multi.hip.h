// epnn_charges_vjp_multi_xyz_cell: charges and g[k]^T dq/dxyz (and the strain derivative) for K cotangents in one pass (kernels and
// arithmetic: epnn_vjp_multi.hip.h).  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_api_grad.hip.h"
#include "epnn_api_jvp.hip.h"
#include "epnn_vjp_multi.hip.h"

// The sweeps carry the cotangents in chunks, the widest instantiated k_gvm_sweep<MODE, KC> that fits what is left (jvm_chunk: K = 7
// runs 4 + 2 + 1); the per-pair and per-atom kernels are chosen by the bucket of K (jvm_bucket).
template <int MODE>
static void gvm_sweep_launch(epnn_handle *h, const GlCall &c, int K, const float *W2, const float *Xres, const float *Xstr, const float *Y,
                             const float *dS, size_t dstride, float *out, size_t ostride) {
    for (int k0 = 0; k0 < K;) {
        const int kc = jvm_chunk(K - k0);
        const float *cd = dS + k0 * dstride;
        float *co = out + k0 * ostride;
        if (kc == 4)
            hipLaunchKernelGGL((k_gvm_sweep<MODE, 4>), dim3(c.nt), dim3(64), 0, h->stream, c.d_tasks, c.d_moff, c.G.A, W2, Xres, Xstr, Y, cd, dstride,
                               co, ostride, (int)c.nt);
        else if (kc == 2)
            hipLaunchKernelGGL((k_gvm_sweep<MODE, 2>), dim3(c.nt), dim3(64), 0, h->stream, c.d_tasks, c.d_moff, c.G.A, W2, Xres, Xstr, Y, cd, dstride,
                               co, ostride, (int)c.nt);
        else
            hipLaunchKernelGGL((k_gvm_sweep<MODE, 1>), dim3(c.nt), dim3(64), 0, h->stream, c.d_tasks, c.d_moff, c.G.A, W2, Xres, Xstr, Y, cd, dstride,
                               co, ostride, (int)c.nt);
        k0 += kc;
    }
}

// The listed pairs' edge gradients gE [K][P1][48] -> their coordinate slots, open molecules or cells (the entry takes no box rows)
template <int KM>
static void launch_gvm_pair_xyz(epnn_handle *h, const GlCall &c, int K, const float *gE, double *slotx, int *bad) {
    geo_dispatch(c.geo.kind, [&](auto kind) {
        if constexpr (decltype(kind)::value != GEO_BOX)
            hipLaunchKernelGGL((k_gvm_pair_xyz<decltype(kind)::value, KM>), dim3((unsigned)((c.np + 255) / 256)), dim3(256), 0, h->stream, c.L, c.np,
                               K, c.P1, 2 * c.P1, c.d_molof, c.d_xyz, c.geo.words(), gE, (double)h->cfg.cutoff, (double)h->cfg.eta,
                               h->d_mu.as<double>(), slotx, bad);
    });
}

// One call: the gradient path's set-up and checkpointed forward (gl_grad_forward; g [K][A] is its staged span, the K-fold cotangent
// buffers its one `more` block, cut up below), then the K-cotangent backward and one download.  The block, every buffer K copies of
// one cotangent's:  gq | gh | ghp | dS | partP | partR | share | out | slotP | slotR | gE | slotx, out = [A] q | [K][A][3] gxyz |
// flag | [K][B][9] gstrain.  The single-cotangent buffers gl_grad_forward places serve the forward; its backward rows stay unused.
static int charges_vjp_multi_impl(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                  const float *Q, const HostGeo &geo, int K, const float *g, float *q_out, float *gxyz_out, float *gstrain_out) {
    if (geo.kind == GEO_BOX) EPNN_FAIL("%s: internal error (box rows: the cotangent kernels take cells)", name);
    GradLarge *gl = grad_large_state(h);
    if (grad_large_weights(h, gl)) return 1;
    const int T = h->cfg.T, A = offsets[B];
    const size_t Kz = (size_t)K, nH = (size_t)A * GL_H, nE = (size_t)A * GL_E;
    const GlSpan span_g{g, Kz * A * 4, false};
    int maxp_i = 1;
    for (int b = 0; b < B; ++b) maxp_i = std::max(maxp_i, gl_pieces(offsets[b + 1] - offsets[b]));
    const size_t maxp = (size_t)maxp_i;
    // the per-atom buffers first, each on a 256-byte step; the per-pair ones behind them, whose sizes gl_grad_forward adds once it has
    // counted the pairs (P1 rows, 2 P1 slots per cotangent): slotP | slotR | gE | slotx
    size_t at = 0;
    auto cut = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~size_t(255); return o; };
    const size_t b_gq = cut(Kz * A * 4), b_gh = cut(Kz * nE * 4), b_ghp = cut(Kz * nE * 4), b_dS = cut(Kz * nH * 4),
                 b_partP = cut(Kz * maxp * nH * 4), b_partR = cut(Kz * maxp * nH * 4), b_share = cut(Kz * A * 48),
                 b_out = cut(((size_t)A + Kz * A * 3 + 1 + Kz * B * 9) * 4);
    const size_t more = at, more_pairs = Kz * (2 * 2 * GL_H * 4 + GL_E * 4 + 2 * 72);
    GlGrad r;
    if (gl_grad_forward(h, gl, name, B, N, offsets, xyz, x, Q, geo, &span_g, 1, &more, 1, false, r, &more_pairs)) return 1;
    const GlCall &c = r.c;
    const size_t P1 = c.P1, SL = 2 * P1;
    const size_t b_slotP = more, b_slotR = b_slotP + Kz * SL * GL_H * 4, b_gE = b_slotR + Kz * SL * GL_H * 4, b_slotx = b_gE + Kz * P1 * GL_E * 4;
    char *blk = c.dw + r.o_more[0];
    auto fp = [&](size_t o) { return reinterpret_cast<float *>(blk + o); };
    float *gq = fp(b_gq), *gh = fp(b_gh), *ghp = fp(b_ghp), *dS = fp(b_dS), *partP = fp(b_partP), *partR = fp(b_partR), *slotP = fp(b_slotP),
          *slotR = fp(b_slotR), *gE = fp(b_gE), *out = fp(b_out);
    double *slotx = reinterpret_cast<double *>(blk + b_slotx), *share = gstrain_out ? reinterpret_cast<double *>(blk + b_share) : nullptr;
    float *q_fin = out, *gx = out + A;
    int *bad = reinterpret_cast<int *>(out + A + Kz * A * 3);
    float *gs = out + A + Kz * A * 3 + 1;
    const int np = c.np;
    const unsigned gP = (unsigned)np, gA = c.gA;
    const GlGeom &G = c.G;
    const GlPairs &L = c.L;
    const int *inc = c.inc;
    const float *d_x = c.d_x, *d_Q = c.d_Q;
    float *hck = r.hck, *Sck = r.Sck, *qck = r.qck, *dP = r.dP, *dR = r.dR, *Yb = r.Yb, *Yc = r.Yc;
    const dim3 w64(64);
    const size_t pstride = maxp * nH;
    const float *feats = hck + T * nE;
    // ---- the seeds: the staged g
    HIPCHK(hipMemcpyAsync(gq, c.d_extra[0], Kz * A * 4, hipMemcpyDeviceToDevice, h->stream));
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
                                   (const float *)dR, (const float *)gq, slotP, slotR, gE);
            });
        jvm_bucket(K, [&](auto km) {
            hipLaunchKernelGGL((k_gvm_epn_atom_bwd<decltype(km)::value>), dim3(A), w64, 0, h->stream, gl->pas[t], G, K, SL, inc, (const float *)slotP,
                               (const float *)slotR, gh, gq);
        });
    }
    HIPCHK(hipGetLastError());
    // ---- backward: GNN steps
    for (int t = T - 1; t >= 0; --t) {
        const float *ht = t ? hck + t * nE : nullptr;
        jvm_bucket(K, [&](auto km) {
            hipLaunchKernelGGL((k_gvm_upd_bwd<decltype(km)::value>), dim3(A), w64, 0, h->stream, gl->msg[t], gl->upd, G, K, ht,
                               (const float *)(Sck + t * nH), (const float *)gh, ghp, dS);
        });
        hipLaunchKernelGGL(k_gl_proj, dim3(A), w64, 0, h->stream, gl->msg[t], G, d_x, ht, (const float *)nullptr, d_Q, dP, dR, Yb, Yc);
        if (t == 0) {                                            // a_i of step 0 is constant: only dG of the listed pairs
            if (np > 0)
                jvm_bucket(K, [&](auto km) {
                    hipLaunchKernelGGL((k_gvm_gnn_pair<decltype(km)::value>), dim3(gP), w64, 0, h->stream, gl->msg[t], L, K, A, P1, SL,
                                       (const float *)dP, (const float *)dR, (const float *)dS, (float *)nullptr, (float *)nullptr, gE);
                });
            break;
        }
        gvm_sweep_launch<1>(h, c, K, gl->msg[t].W2, dP, dR, Yb, dS, nH, partP, pstride);
        gvm_sweep_launch<2>(h, c, K, gl->msg[t].W2, dR, dP, Yc, dS, nH, partR, pstride);
        if (np > 0)
            jvm_bucket(K, [&](auto km) {
                hipLaunchKernelGGL((k_gvm_gnn_pair<decltype(km)::value>), dim3(gP), w64, 0, h->stream, gl->msg[t], L, K, A, P1, SL, (const float *)dP,
                                   (const float *)dR, (const float *)dS, slotP, slotR, gE);
            });
        jvm_bucket(K, [&](auto km) {
            hipLaunchKernelGGL((k_gvm_gnn_atom_bwd<decltype(km)::value>), dim3(A), w64, 0, h->stream, gl->msg[t], G, K, pstride, SL, inc,
                               (const float *)partP, (const float *)partR, (const float *)slotP, (const float *)slotR, (const float *)dP,
                               (const float *)dS, ghp);
        });
        std::swap(gh, ghp);
    }
    HIPCHK(hipGetLastError());
    // ---- edges -> coordinates
    if (np > 0) jvm_bucket(K, [&](auto km) { launch_gvm_pair_xyz<decltype(km)::value>(h, c, K, gE, slotx, bad); });
    hipLaunchKernelGGL(k_gvm_atom_xyz, dim3(gA, (unsigned)K), dim3(256), 0, h->stream, A, SL, inc, (const double *)slotx, gx, share);
    if (share) hipLaunchKernelGGL(k_gvm_strain_mol, dim3((unsigned)B, (unsigned)K), dim3(64), 0, h->stream, A, (const double *)share, c.d_moff, gs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(q_fin, qck + (size_t)T * A, (size_t)A * 4, hipMemcpyDeviceToDevice, h->stream));
    // ---- one download: q | gxyz[K] | flag | gstrain[K]
    const size_t o_flag = (size_t)A + Kz * A * 3, nback = o_flag + 1 + (gstrain_out ? Kz * B * 9 : 0);
    if (gl->pin_out.ensure(nback * 4)) return 1;
    float *back = gl->pin_out.as<float>();
    HIPCHK(hipMemcpyAsync(back, out, nback * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int flag = reinterpret_cast<const int *>(back)[o_flag];
    if (flag & 2) EPNN_FAIL("%s: the pair list is not symmetric", name);
    if (flag != 0)
        EPNN_FAIL("%s: two atoms of a molecule%s coincide (distance 0: the edge features have no derivative there)", name,
                  geo.periodic() ? " or their periodic images" : "");
    memcpy(q_out, back, (size_t)A * 4);
    memcpy(gxyz_out, back + A, Kz * A * 12);
    if (gstrain_out) memcpy(gstrain_out, back + o_flag + 1, Kz * B * 36);
    return 0;
}

extern "C" int epnn_charges_vjp_multi_xyz_cell(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                               const float *Q, const float *cell, int K, const float *g, float *q_out, float *gxyz_out,
                                               float *gstrain_out) {
    const char *name = "epnn_charges_vjp_multi_xyz_cell";
    if (K < 1 || K > GVM_MAXK) EPNN_FAIL("%s: K must be in 1..%d, got %d", name, GVM_MAXK, K);
    if (!g) EPNN_FAIL("%s: null argument", name);
    GeoArg arg;
    // the checks and the settling of the forward-mode entries (a null pointer, the batch, a fused-only handle, the cell, update
    // layers, a partitioned handle; a begun forward is finished, a training step in flight waited for, the weights packed)
    if (charges_jvp_enter(h, name, B, N, offsets, xyz, x, Q, cell, K, q_out, gxyz_out, arg)) return 1;
    return charges_vjp_multi_impl(h, name, B, N, offsets, xyz, x, Q, arg.geo, K, g, q_out, gxyz_out, gstrain_out);
}
