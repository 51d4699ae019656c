// epnn_coulomb_xyz: charges, electrostatic potential, Coulomb energy and total forces of a flat coordinate batch in one call
// (kernels: epnn_coulomb.hip.h).  The pair-list gradient call (epnn_api_grad.hip.h) with its seed made on the device: set-up and
// checkpointed forward, the Coulomb sweep on that forward's charges (phi = dE/dq into the seed), the shared backward, one download.
// Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_api_grad.hip.h"
#include "epnn_api_jvp.hip.h"
#include "epnn_coulomb.hip.h"

// The sweep's tasks (k_cl_sweep): molecules of up to CL_BLOCK atoms whole and packed in batch order while they fit one wavefront,
// larger ones as blocks of CL_BLOCK atoms times cl_pieces(n) pieces of their partner range.  Returns the most pieces of a molecule.
static int cl_build_tasks(int B, const int32_t *offsets, std::vector<int4> &tasks) {
    int maxp = 1;
    for (int b = 0; b < B;) {
        const int lo = offsets[b], hi = offsets[b + 1], n = hi - lo;
        if (n <= CL_BLOCK) {
            int b1 = b + 1;
            while (b1 < B && offsets[b1 + 1] - offsets[b1] <= CL_BLOCK && offsets[b1 + 1] - lo <= CL_BLOCK) ++b1;
            tasks.push_back(make_int4(lo, offsets[b1] - lo, lo, offsets[b1]));
            b = b1;
            continue;
        }
        const int np = cl_pieces(n), len = (n + np - 1) / np;
        maxp = std::max(maxp, np);
        for (int a0 = lo; a0 < hi; a0 += CL_BLOCK)
            for (int k = 0; k < np; ++k) {
                const int p0 = std::min(lo + k * len, hi), p1 = std::min(p0 + len, hi);
                tasks.push_back(make_int4(a0, std::min(CL_BLOCK, hi - a0) | (k << 8), p0, p1));
            }
        ++b;
    }
    return maxp;
}

static int coulomb_impl(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                        const float *Q, const HostGeo &geo, double ke, double alpha, float *q_out, float *phi_out, double *e_out, float *f_out, float *ffix_out,
                        float *fq_out) {
    GradLarge *gl = grad_large_state(h);
    if (grad_large_weights(h, gl)) return 1;
    const int T = h->cfg.T, A = offsets[B];
    std::vector<int4> tasks;
    const size_t cpieces = (size_t)cl_build_tasks(B, offsets, tasks);
    const GlSpan span_t{tasks.data(), tasks.size() * sizeof(int4), false};
    // [A] phi | [A][3] ffix | flag, then [B] E in float64: directly behind the backward's output block, one download for both;
    // the sweep's partial rows [pieces][A][4] and the atoms' energy shares [A], float64
    const size_t o_E = (((size_t)A * 4 + 1) * 4 + 7) & ~size_t(7), co_bytes = o_E + (size_t)B * 8;
    const size_t more[2] = {co_bytes, (cpieces * 4 + 1) * (size_t)A * 8};
    GlGrad r;
    if (gl_grad_forward(h, gl, name, B, N, offsets, xyz, x, Q, geo, &span_t, 1, more, 2, false, r)) return 1;
    const GlCall &c = r.c;
    char *co = c.dw + r.o_more[0];
    float *phi = reinterpret_cast<float *>(co), *ffix = phi + A;
    int *hit = reinterpret_cast<int *>(phi + 4 * (size_t)A);
    double *E = reinterpret_cast<double *>(co + o_E), *part = reinterpret_cast<double *>(c.dw + r.o_more[1]),
           *share = part + cpieces * 4 * (size_t)A;
    const float *q_dev = r.qck + (size_t)T * A;
    const int4 *d_ctasks = reinterpret_cast<const int4 *>(c.d_extra[0]);
    // ---- the Coulomb sweep on the forward's own charges: phi is the backward's seed
    HIPCHK(hipMemsetAsync(hit, 0, 4, h->stream));
    if (alpha > 0.0)
        hipLaunchKernelGGL(k_cl_sweep<true>, dim3((unsigned)tasks.size()), dim3(64), 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz, q_dev,
                           A, (float)alpha, part, hit);
    else
        hipLaunchKernelGGL(k_cl_sweep<false>, dim3((unsigned)tasks.size()), dim3(64), 0, h->stream, d_ctasks, c.d_moff, c.d_molof, c.d_xyz, q_dev,
                           A, 0.f, part, hit);
    hipLaunchKernelGGL(k_cl_atom, dim3(c.gA), dim3(256), 0, h->stream, A, c.d_moff, c.d_molof, q_dev, (const double *)part, ke, r.gq, phi, ffix,
                       share);
    hipLaunchKernelGGL(k_cl_energy, dim3((unsigned)B), dim3(64), 0, h->stream, (const double *)share, c.d_moff, E);
    HIPCHK(hipGetLastError());
    if (gl_grad_backward(h, gl, r, B, false)) return 1;
    // ---- one download: q | gxyz | flag | (the unused strain rows and the step to the next buffer) | phi | ffix | flag | E
    const char *from = reinterpret_cast<const char *>(r.q_fin);
    const size_t nbytes = (size_t)(co + co_bytes - from), at_co = (size_t)(co - from);
    if (gl->pin_out.ensure(nbytes)) return 1;
    char *back = gl->pin_out.as<char>();
    HIPCHK(hipMemcpyAsync(back, from, nbytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const float *bq = reinterpret_cast<const float *>(back), *bgx = bq + A, *bphi = reinterpret_cast<const float *>(back + at_co),
                *bffix = bphi + A;
    const int flag = reinterpret_cast<const int *>(bq)[4 * (size_t)A], chit = reinterpret_cast<const int *>(bphi)[4 * (size_t)A];
    if (flag & 2) EPNN_FAIL("%s: the pair list is not symmetric", name);
    if (flag != 0 || chit != 0) EPNN_FAIL("%s: two atoms of a molecule coincide (distance 0: neither the Coulomb terms nor the edge features have a derivative there)", name);
    memcpy(q_out, bq, (size_t)A * 4);
    memcpy(phi_out, bphi, (size_t)A * 4);
    memcpy(e_out, back + at_co + o_E, (size_t)B * 8);
    for (size_t k = 0; k < 3 * (size_t)A; ++k) {
        const float fq = -bgx[k];
        f_out[k] = bffix[k] + fq;
        if (fq_out) fq_out[k] = fq;
    }
    if (ffix_out) memcpy(ffix_out, bffix, (size_t)A * 12);
    return 0;
}

extern "C" int epnn_coulomb_xyz(epnn_handle *h, int B, int N, const int32_t *offsets, const float *xyz, const float *x, const float *Q,
                                double ke, double alpha, float *q_out, float *phi_out, double *e_out, float *f_out, float *ffix_out,
                                float *fq_out) {
    const char *name = "epnn_coulomb_xyz";
    if (!phi_out || !e_out) EPNN_FAIL("%s: null argument", name);
    // (the library is built with -ffinite-math-only: std::isfinite would fold to true, and so would a test of an argument's own
    //  bits -- the tests below read them back from volatile words, of which the compiler assumes nothing)
    volatile uint64_t seen[2];
    uint64_t kbits, abits;
    memcpy(&kbits, &ke, 8);
    memcpy(&abits, &alpha, 8);
    seen[0] = kbits; seen[1] = abits;
    kbits = seen[0]; abits = seen[1];
    const uint64_t expo = 0x7ff0000000000000ull;
    if ((kbits & expo) == expo) EPNN_FAIL("%s: ke must be finite", name);
    if ((abits & expo) == expo || ((abits >> 63) && (abits << 1)))
        EPNN_FAIL("%s: alpha must be finite and not negative (0: bare Coulomb)", name);
    GeoArg arg;                                                  // (open molecules: the entry takes no cell)
    if (charges_jvp_enter(h, name, B, N, offsets, xyz, x, Q, nullptr, 1, q_out, f_out, arg)) return 1;
    return coulomb_impl(h, name, B, N, offsets, xyz, x, Q, arg.geo, ke, alpha, q_out, phi_out, e_out, f_out, ffix_out, fq_out);
}
