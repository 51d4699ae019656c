// The geometry of one call on the host -- open molecules, box rows [B][3] or EpnnCell records [B] -- as ONE value that every internal
// function takes, and the front-end's launches that choose a kernel's entry point by it.  Part of the one translation unit epnn_api.hip.
#pragma once
#include "epnn_host.h"
#include "epnn_frontend.hip.h"

// Box rows of a periodic forward (include/epnn.h): finite, >= 0, and a periodic length of at least twice the cutoff
static int check_box(int B, const float *box, double cutoff, const char *what) {
    if (!box) EPNN_FAIL("%s: null box", what);
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 3; ++k) {
            const float L = box[3 * b + k];
            uint32_t bits;                        // (the library is built with -ffinite-math-only: std::isfinite would fold to true)
            memcpy(&bits, &L, 4);
            if ((bits & 0x7f800000u) == 0x7f800000u || L < 0.f)
                EPNN_FAIL("%s: box[%d][%d] = %g: a length must be finite and >= 0 (0: open axis)", what, b, k, (double)L);
            if (L > 0.f && (double)L < 2.0 * cutoff)
                EPNN_FAIL("%s: box[%d][%d] = %g is shorter than twice the cutoff (%g)", what, b, k, (double)L, 2.0 * cutoff);
        }
    return 0;
}

// General cells (include/epnn.h): validates cell [B][3][3] and prepares what the device needs of every molecule (EpnnCell: the
// entries, the dual vectors in float64, the constants of the front-end's float32 pre-test).  Refused, naming molecule and axis: a
// NaN or infinite entry, linearly dependent non-zero rows, a periodic axis whose perpendicular width 1 / |g_k| is below 2 * cutoff.
static int check_cell(int B, const float *cell, double cutoff, const char *what, std::vector<EpnnCell> &out) {
    if (!cell) EPNN_FAIL("%s: null cell", what);
    out.assign((size_t)B, EpnnCell());
    for (int b = 0; b < B; ++b) {
        EpnnCell &c = out[b];
        memset(&c, 0, sizeof(c));
        double a[3][3], g[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, len[3];
        int per[3], m = 0;
        for (int k = 0; k < 3; ++k) {
            bool nz = false;
            for (int x = 0; x < 3; ++x) {
                const float v = cell[9 * b + 3 * k + x];
                uint32_t bits;                    // (-ffinite-math-only: std::isfinite would fold to true)
                memcpy(&bits, &v, 4);
                if ((bits & 0x7f800000u) == 0x7f800000u)
                    EPNN_FAIL("%s: cell[%d][%d][%d] is not finite (molecule %d, axis %d)", what, b, k, x, b, k);
                a[k][x] = (double)v;
                c.a[3 * k + x] = v;
                nz = nz || v != 0.f;
            }
            len[k] = sqrt(a[k][0] * a[k][0] + a[k][1] * a[k][1] + a[k][2] * a[k][2]);
            if (nz) per[m++] = k;
        }
        auto cross = [](const double *u, const double *v, double *o) {
            o[0] = u[1] * v[2] - u[2] * v[1]; o[1] = u[2] * v[0] - u[0] * v[2]; o[2] = u[0] * v[1] - u[1] * v[0];
        };
        auto dot = [](const double *u, const double *v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; };
        if (m == 3) {
            double c12[3], c20[3], c01[3];
            cross(a[1], a[2], c12); cross(a[2], a[0], c20); cross(a[0], a[1], c01);
            const double det = dot(a[0], c12);
            if (!(fabs(det) > 1e-12 * len[0] * len[1] * len[2]))
                EPNN_FAIL("%s: the rows of cell[%d] (molecule %d) are linearly dependent (axis 2 lies in the plane of axes 0 and 1)", what, b, b);
            for (int x = 0; x < 3; ++x) { g[0][x] = c12[x] / det; g[1][x] = c20[x] / det; g[2][x] = c01[x] / det; }
        } else if (m == 2) {
            const int p = per[0], q = per[1];
            double n[3], t[3];
            cross(a[p], a[q], n);
            const double n2 = dot(n, n);
            if (!(sqrt(n2) > 1e-12 * len[p] * len[q]))
                EPNN_FAIL("%s: rows %d and %d of cell[%d] (molecule %d) are linearly dependent (axis %d is parallel to axis %d)", what, p, q, b, b, q, p);
            cross(a[q], n, t);
            for (int x = 0; x < 3; ++x) g[p][x] = t[x] / n2;
            cross(n, a[p], t);
            for (int x = 0; x < 3; ++x) g[q][x] = t[x] / n2;
        } else if (m == 1) {
            const int p = per[0];
            for (int x = 0; x < 3; ++x) g[p][x] = a[p][x] / (len[p] * len[p]);
        }
        double S = 0.0, wmin = 0.0;
        for (int i = 0; i < m; ++i) {
            const int k = per[i];
            const double w = 1.0 / sqrt(dot(g[k], g[k]));
            if (!(w >= 2.0 * cutoff))
                EPNN_FAIL("%s: cell[%d] (molecule %d): the perpendicular width of periodic axis %d is %g, below twice the cutoff (%g)", what, b, b,
                          k, w, 2.0 * cutoff);
            S += len[k];
            wmin = i == 0 ? w : std::min(wmin, w);
        }
        for (int k = 0; k < 3; ++k)
            for (int x = 0; x < 3; ++x) c.g[3 * k + x] = g[k][x];
        // the front-end's pre-test (front_scan_row): X bounds the components of a pre-tested position (S, plus 1024 A along open
        // directions where there are any), u = 2^-24, pre_eps = 32 u X / w, margin 1.0001 + 96 r + 1024 r^2, r = u X / cutoff
        const double X = S + (m < 3 ? 1024.0 : 0.0), r = 0x1p-24 * X / cutoff;
        c.pre_ext = (float)X;
        c.pre_eps = m ? (float)std::min(0.5, 32.0 * 0x1p-24 * X / wmin * 1.000001) : 0.f;
        c.pre_margin = (float)((1.0001 + r * (96.0 + 1024.0 * r)) * 1.000001);
    }
    return 0;
}

// Kind (epnn_host.h) and one untyped pointer to the rows, cast by the accessors alone.  HostGeo: rows in host memory (the caller's box
// rows, a GeoArg's records); DevGeo: rows on the device (staged with the call's inputs).  A default-constructed one is open molecules.
namespace {                       // (internal linkage: the library exports its C ABI only)
template <bool ON_DEVICE>
struct GeoRows {
    GeoKind kind = GEO_OPEN;
    const void *rows = nullptr;
    size_t row_bytes() const { return kind == GEO_CELL ? sizeof(EpnnCell) : kind == GEO_BOX ? 3 * sizeof(float) : 0; }
    size_t bytes(int B) const { return (size_t)B * row_bytes(); }
    bool periodic() const { return kind != GEO_OPEN; }
    const char *raw() const { return static_cast<const char *>(rows); }          // the rows as bytes, for copies
    const float *box() const { return static_cast<const float *>(rows); }
    const EpnnCell *cells() const { return static_cast<const EpnnCell *>(rows); }
    const float *words() const { return static_cast<const float *>(rows); }      // either kind's rows as the GeoKind-templated kernels take them
};
using HostGeo = GeoRows<false>;
using DevGeo = GeoRows<true>;
// What an extern "C" entry makes of its `box` or `cell` argument, checked under the entry's name (a cell's records live here)
struct GeoArg {
    HostGeo geo;
    std::vector<EpnnCell> records;
    int box(int B, const float *box, double cutoff, const char *what) { geo = HostGeo{GEO_BOX, box}; return check_box(B, box, cutoff, what); }
    int cell(int B, const float *cell, double cutoff, const char *what) {
        if (check_cell(B, cell, cutoff, what, records)) return 1;
        geo = HostGeo{GEO_CELL, records.data()};
        return 0;
    }
};
}
// the same geometry with its rows at `d_rows` on the device (open molecules have none)
static inline DevGeo geo_on_device(const HostGeo &g, const void *d_rows) { return DevGeo{g.kind, g.periodic() ? d_rows : nullptr}; }

// A runtime kind as a compile-time constant, f(std::integral_constant<int, kind>): for the kernels templated on the GeoKind (rows: words())
template <class F>
static inline void geo_dispatch(GeoKind kind, F &&f) {
    if (kind == GEO_CELL) f(std::integral_constant<int, GEO_CELL>{});
    else if (kind == GEO_BOX) f(std::integral_constant<int, GEO_BOX>{});
    else f(std::integral_constant<int, GEO_OPEN>{});
}

// ---- the front-end's kernel families, each launched at the entry point of the geometry's kind.  The two passes of the pair list
// (a workgroup per four atoms): the rows' counts with their prefix sums, then the pairs' records with their incidence links
static inline void launch_front_count(epnn_handle *h, const FrontArgs &F, const DevGeo &g) {
    const dim3 rows((unsigned)((F.A + 3) / 4)), block(256);
    if (g.kind == GEO_CELL) hipLaunchKernelGGL(k_front_count_cell, rows, block, 0, h->stream, F, g.cells());
    else if (g.kind == GEO_BOX) hipLaunchKernelGGL(k_front_count_pbc, rows, block, 0, h->stream, F, g.box());
    else hipLaunchKernelGGL(k_front_count, rows, block, 0, h->stream, F);
    hipLaunchKernelGGL(k_front_scan_both, dim3(1), dim3(1024), 0, h->stream, F);
}
static inline void launch_front_fill(epnn_handle *h, const FrontArgs &F, const DevGeo &g) {
    const dim3 rows((unsigned)((F.A + 3) / 4)), block(256);
    if (g.kind == GEO_CELL) hipLaunchKernelGGL(k_front_fill_cell, rows, block, 0, h->stream, F, g.cells());
    else if (g.kind == GEO_BOX) hipLaunchKernelGGL(k_front_fill_pbc, rows, block, 0, h->stream, F, g.box());
    else hipLaunchKernelGGL(k_front_fill, rows, block, 0, h->stream, F);
    hipLaunchKernelGGL(k_front_link, dim3((unsigned)std::min<size_t>(((size_t)F.pcap + 255) / 256, 1024)), block, 0, h->stream, F);
}
static inline void launch_edges_dense(epnn_handle *h, unsigned grid, const float *xyz, const DevGeo &g, int n, int num, double cutoff,
                                      double eta, const double *mu, float *e_out, double *c_out) {
    if (g.kind == GEO_CELL) hipLaunchKernelGGL(k_edges_dense_cell, dim3(grid), dim3(256), 0, h->stream, xyz, g.cells(), n, num, cutoff, eta, mu, e_out, c_out);
    else if (g.kind == GEO_BOX) hipLaunchKernelGGL(k_edges_dense_pbc, dim3(grid), dim3(256), 0, h->stream, xyz, g.box(), n, num, cutoff, eta, mu, e_out, c_out);
    else hipLaunchKernelGGL(k_edges_dense, dim3(grid), dim3(256), 0, h->stream, xyz, n, num, cutoff, eta, mu, e_out, c_out);
}
