// epnn_charges_vjp_multi_xyz_cell: charges and g[k]^T dq/dxyz (and the strain derivative) for K cotangents in one pass (kernels and
// arithmetic: epnn_vjp_multi.hip.h; the backward's driver: gl_grad_backward, epnn_api_grad.hip.h).  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_api_grad.hip.h"
#include "epnn_api_jvp.hip.h"

// One call: the gradient path's set-up, K-fold backward rows and checkpointed forward (gl_grad_forward; g [K][A] is its staged span), the
// seeds, the one backward (gl_grad_backward) and one download: q | [K][A][3] gxyz | flag | [K][B][9] gstrain.
static int charges_vjp_multi_impl(epnn_handle *h, const char *name, int B, int N, const int32_t *offsets, const float *xyz, const float *x,
                                  const float *Q, const HostGeo &geo, int K, const float *g, float *q_out, float *gxyz_out, float *gstrain_out) {
    if (geo.kind == GEO_BOX) EPNN_FAIL("%s: internal error (box rows: the cotangent kernels take cells)", name);
    GradLarge *gl = grad_large_state(h);
    if (grad_large_weights(h, gl)) return 1;
    const int A = offsets[B];
    const size_t Kz = (size_t)K;
    const GlSpan span_g{g, Kz * A * 4, false};
    GlGrad r;
    if (gl_grad_forward(h, gl, name, B, N, offsets, xyz, x, Q, geo, K, &span_g, 1, nullptr, 0, false, r)) return 1;
    HIPCHK(hipMemcpyAsync(r.gq, r.c.d_extra[0], Kz * A * 4, hipMemcpyDeviceToDevice, h->stream));      // the seeds: the staged g
    if (gl_grad_backward(h, gl, r, B, K, gstrain_out != nullptr)) return 1;
    const size_t o_flag = (size_t)A + Kz * A * 3, nback = o_flag + 1 + (gstrain_out ? Kz * B * 9 : 0);
    if (gl->pin_out.ensure(nback * 4)) return 1;
    float *back = gl->pin_out.as<float>();
    HIPCHK(hipMemcpyAsync(back, r.q_fin, nback * 4, hipMemcpyDeviceToHost, h->stream));
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
