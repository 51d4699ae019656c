// How every kernel behind the front-end measures a pair: the image of the float64 displacement, the distance and an edge's radial terms,
// once, on the front-end's primitives (epnn_mic, epnn_mic_cell, EpnnCellD): the paths agree bit for bit by construction.  Part of epnn_api.hip.
#pragma once
#include "epnn_frontend.hip.h"

// One molecule's geometry in registers, GEO as GeoKind (epnn_host.h): 0 open (nothing), 1 box (three lengths, 0 an open axis), 2 cell
// (dual and lattice vectors).  rows: the batch's box rows [B][3] or EpnnCell records [B] in device memory (open: unused, may be null).
//   load_uniform  b is the same in every lane (scalar loads; a cell through readfirstlane).  Where b differs between lanes it
//                 silently hands every lane the first lane's cell: use load_lane there (b = mol_of[i] of the lane's own atom or pair).
//   image         the displacement that the kind's contract names, in place.
template <int GEO>
struct PairGeo {
    __device__ __forceinline__ void load_uniform(const void *, int) {}
    __device__ __forceinline__ void load_lane(const void *, int) {}
    __device__ __forceinline__ void image(double &, double &, double &) const {}
};
template <>
struct PairGeo<1> {
    double L[3];
    __device__ __forceinline__ void load_uniform(const void *rows, int b) { load_lane(rows, b); }      // (a uniform b: scalar loads)
    __device__ __forceinline__ void load_lane(const void *rows, int b) {
        for (int k = 0; k < 3; ++k) L[k] = (double)static_cast<const float *>(rows)[3 * b + k];
    }
    __device__ __forceinline__ void image(double &dx, double &dy, double &dz) const {
        dx = epnn_mic(dx, L[0]); dy = epnn_mic(dy, L[1]); dz = epnn_mic(dz, L[2]);
    }
};
template <>
struct PairGeo<2> : EpnnCellD {       // (its pre-test constant `ext` is not loaded per lane and not used here)
    __device__ __forceinline__ void load_uniform(const void *rows, int b) { load(static_cast<const EpnnCell *>(rows), b); }
    __device__ __forceinline__ void load_lane(const void *rows, int b) {
        const EpnnCell &c = static_cast<const EpnnCell *>(rows)[b];
#pragma unroll
        for (int k = 0; k < 9; ++k) { g[k] = c.g[k]; a[k] = (double)c.a[k]; }
    }
    __device__ __forceinline__ void image(double &dx, double &dy, double &dz) const { epnn_mic_cell(dx, dy, dz, g, a); }
};

// D as scipy.spatial.distance_matrix on coordinates promoted to float64 (epnn_dist): sqrt((dx dx + dy dy) + dz dz), nothing contracted
__device__ __forceinline__ double pair_dist(double dx, double dy, double dz) {
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
}

// The radial terms of an edge (get_init_edges): e_k = C exp(-eta u^2), de_k/dD = (dC - 2 eta u C) exp(-eta u^2) with u = D - mu_k,
// C = (cos(pi D / cutoff) + 1) / 2 and dC = dC/dD.  Raw: D >= cutoff, D <= 0 and i == j are the callers' to guard.  The build contracts
// floating-point expressions, so each keeps the shape the kernels always had, and a caller multiplies slope and gauss in its own order.
constexpr double edge_pi = 3.141592653589793;
__device__ __forceinline__ double edge_cut(double D, double cutoff) { return (cos(edge_pi * D / cutoff) + 1.0) / 2.0; }
__device__ __forceinline__ double edge_dcut(double D, double cutoff) { return -0.5 * (edge_pi / cutoff) * sin(edge_pi * D / cutoff); }
__device__ __forceinline__ double edge_gauss(double u, double eta) { return exp(-eta * (u * u)); }
__device__ __forceinline__ double edge_slope(double C, double dC, double u, double eta) { return dC - 2.0 * eta * u * C; }
