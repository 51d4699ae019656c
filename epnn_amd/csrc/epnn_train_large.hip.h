// Training step from the pair list (option "train_path" = 2): the kernels that turn the backward of epnn_grad_large.hip.h into
// weight gradients.  Part of the one translation unit epnn_api.hip.
//
// The backward kernels of the gradient path already form every activation gradient of the factorised model; a training step asks them
// to keep the rows a weight gradient is an outer product of (GlTape) and sums those products here:
//
//   per atom           update MLP (u0 x d1, u1 x d2, u2 x gh; shared by the T steps, so every step adds), W3 / b3 of a message MLP
//                      (S x dM, N dM), the Wi / Wj blocks and b1 of a first Dense (a x dP, a x dR, dP), and the (N - n) padded
//                      partners' share of W2 / b2 (relu(P) x (N - n) d2)
//   per listed pair    the We block (e x (dz1_ij + dz1_ji)), the near-pair corrections' share of W2 / b2 (with G minus without),
//                      and W2, b2, W3 of a pass MLP for both orders of the pair (b3 of a pass MLP cancels between the two orders)
//   all pairs          W2 / b2 of a message MLP: inside the row pass of the sweep (k_gl_sweep<1, 1, 1>), on the matrix pipe
//
// Every product is a job of k_tl_outer: rows [r] of X (K wide) and Y (O wide) -> sum_r X_r (x) Y_r and sum_r Y_r.  A job's rows are
// cut into TL_G runs, one workgroup each, a thread owns up to TL_EPT entries of the result and adds its run's rows in order; the TL_G
// partial results are added in order by k_tl_reduce.  Nothing is atomic: the gradient is bit-reproducible, and the scratch is the
// kept rows (O(atoms + listed pairs)) plus partials of constant size.
#pragma once
#include "epnn_grad_large.hip.h"

#define TL_G 128                  // runs (workgroups) per job
#define TL_PS 2624                // floats per partial: the largest job is u0 x d1, 80 * 32 + 32
#define TL_EPT 11                 // entries per thread: ceil(TL_PS / 256)
#define TL_ROWS 8                 // rows staged in LDS at a time
#define TL_MAXJOBS 10
#define TL_NW 4096                // most wavefronts of a weight-gradient sweep (each leaves one 32 x 32 + 32 partial)

struct TlJob {
    const float *X, *Y;           // rows [rows][xs], [rows][ys]; X null with K = 0: the column sums of Y alone
    int K, O, xs, ys;
    long long rows;
};
struct TlJobs {
    TlJob j[TL_MAXJOBS];
};
// part [job][TL_G][TL_PS]: entry k * O + f = sum_r X[r][k] Y[r][f], entry K * O + f = sum_r Y[r][f]
__global__ __launch_bounds__(256) void k_tl_outer(TlJobs J, float *part) {
    __shared__ float xs[TL_ROWS][84], ys[TL_ROWS][48];
    const TlJob jb = J.j[blockIdx.y];
    const int tid = threadIdx.x, ne = jb.K * jb.O + jb.O;
    const long long run = (jb.rows + TL_G - 1) / TL_G;
    const long long r0 = min(jb.rows, (long long)blockIdx.x * run), r1 = min(jb.rows, r0 + run);
    float acc[TL_EPT];
    int ek[TL_EPT], ef[TL_EPT];
#pragma unroll
    for (int m = 0; m < TL_EPT; ++m) {
        const int idx = min(tid + 256 * m, ne - 1);
        acc[m] = 0.f;
        ek[m] = idx / jb.O;
        ef[m] = idx - ek[m] * jb.O;
    }
    for (long long r = r0; r < r1; r += TL_ROWS) {
        const int nr = (int)min((long long)TL_ROWS, r1 - r);
        __syncthreads();
        for (int k = tid; k < nr * (jb.K + 1); k += 256) {
            const int rr = k / (jb.K + 1), kk = k - rr * (jb.K + 1);
            xs[rr][kk] = kk < jb.K ? jb.X[(size_t)(r + rr) * jb.xs + kk] : 1.f;
        }
        for (int k = tid; k < nr * jb.O; k += 256) {
            const int rr = k / jb.O, ff = k - rr * jb.O;
            ys[rr][ff] = jb.Y[(size_t)(r + rr) * jb.ys + ff];
        }
        __syncthreads();
        for (int rr = 0; rr < nr; ++rr)
#pragma unroll
            for (int m = 0; m < TL_EPT; ++m) acc[m] = fmaf(xs[rr][ek[m]], ys[rr][ef[m]], acc[m]);
    }
    float *o = part + ((size_t)blockIdx.y * TL_G + blockIdx.x) * TL_PS;
#pragma unroll
    for (int m = 0; m < TL_EPT; ++m)
        if (tid + 256 * m < ne) o[tid + 256 * m] = acc[m];
}

// grad[dst + i] += scale * sum over the nblk partials (in order: four quarters, each in order, then the quarters in order) of
// part[src + blk * stride + i], i < len.  One entry per blockIdx.y; the entries of one launch have distinct destinations.
#define TL_MAXRED 20
struct TlRed {
    int dst[TL_MAXRED], len[TL_MAXRED], nblk[TL_MAXRED], stride[TL_MAXRED];
    long long src[TL_MAXRED];
    float scale[TL_MAXRED];
};
__global__ __launch_bounds__(1024) void k_tl_reduce(TlRed R, const float *part, float *grad) {
    __shared__ float q[16][64];
    const int e = blockIdx.y, i = blockIdx.x * 64 + (threadIdx.x & 63), s = threadIdx.x >> 6;
    const int len = R.len[e], nb = R.nblk[e], per = (nb + 15) / 16;
    float sum = 0.f;
    if (i < len)
        for (int b = s * per; b < min(nb, (s + 1) * per); ++b) sum += part[R.src[e] + (size_t)b * R.stride[e] + i];
    q[s][threadIdx.x & 63] = sum;
    __syncthreads();
    if (s == 0 && i < len) {
        float t = 0.f;
        for (int k = 0; k < 16; ++k) t += q[k][threadIdx.x];
        grad[R.dst[e] + i] += R.scale[e] * t;
    }
}

// the input rows of a first Dense: a = [x | h | q] (h null: zeros; q null: Q / n), [A][64] with zeros behind the F columns
__global__ __launch_bounds__(256) void k_tl_arow(GlGeom G, const float *x, const float *h, const float *q, const float *Q, float *arow) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)G.A * 64) return;
    const int a = (int)(idx >> 6), k = (int)(idx & 63);
    float v = 0.f;
    if (k < G.nx) v = x[(size_t)a * G.nx + k];
    else if (k < G.nx + GL_E) v = h ? h[(size_t)a * GL_E + (k - G.nx)] : 0.f;
    else if (k == G.nx + GL_E) {
        const int b = G.mol_of[a];
        v = q ? q[a] : Q[b] / (float)(G.moff[b + 1] - G.moff[b]);
    }
    arow[idx] = v;
}

// the seed of the backward and the loss terms: gq = 2 (q - y), term = (y - q)^2
__global__ __launch_bounds__(256) void k_tl_seed(int A, const float *q, const float *y, float *gq, float *term) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const float d = q[a] - y[a];
    gq[a] = 2.f * d;
    term[a] = d * d;
}
// a listed pair without both incidence slots would be a front-end fault: the pair kernels skip it, the step must not pass
__global__ __launch_bounds__(256) void k_tl_check_pairs(GlPairs L, int npairs, int *bad) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < npairs && (L.dest_i[p] < 0 || L.dest_j[p] < 0)) atomicOr(bad, 2);
}
